"""CPU oracle for target bootstrapping: the reference's closed forms, restated.

TEST INFRASTRUCTURE ONLY: imported by tests/ (and nothing else).  The product computes the same targets on the
GPU from the Gram matrix of the selected rows (csrc/vq_boot.hip, Woodbury form); this file keeps the reference's own
explicit 1024x1024 inverses so that the two routes check each other.

Parity status: PINNED.  oracle/gen_golden_bootstrap.py runs the reference's ``TargetClip`` itself and records its
targets under tests/golden/bootstrap*.{json,npz}; tests/test_bootstrap_oracle.py checks every function here against
them.  Line numbers refer to src/models/target_clip.py of the reference.

For the kernel's own accuracy (tests/test_bootstrap_edges_*.py): ``exact_target`` / ``exact_target_explicit`` evaluate the
closed forms in rational arithmetic, ``kernel_order_target`` restates the kernel operation for operation (it reproduces
the device's bits and counts the row swaps), ``woodbury_target`` is the Gram route on BLAS / LAPACK.
"""
from __future__ import annotations

import math
import random
from fractions import Fraction
from typing import Dict, List, Mapping, Sequence

import numpy as np


def random_fraction(n_items: int, fraction, replacement: bool) -> List[int]:
    """target_clip.py:297-309: positions to keep -- sample / choices, then ``list(set(...))`` (unique, set order)."""
    tmatches = round(n_items * fraction)
    tmatches = max(tmatches, 1)
    if replacement is False:
        tsamples = random.sample(range(n_items), tmatches)
    else:
        tsamples = random.choices(range(n_items), k=tmatches)
    return list(set(tsamples))


def bootstrap_valid(X_rows: np.ndarray) -> np.ndarray:
    """target_clip.py:192-197: rows = validated matches [m][D]; w = X (X^T X)^-1 1 with X = rows^T."""
    X = np.asarray(X_rows, dtype=np.float64).T
    M = np.matmul(X.T, X)
    M_inv = np.linalg.inv(M)
    mu = np.sum(M_inv, axis=1).reshape([-1, 1])
    return np.dot(X, mu).T[0]


def bootstrap_valid_invalid(X_rows: np.ndarray, Y_rows: np.ndarray, mu: float) -> np.ndarray:
    """target_clip.py:245-260 with X [m][D] validated matches, Y [n][D] validated non-matches."""
    X = np.asarray(X_rows, dtype=np.float64)
    Y = np.asarray(Y_rows, dtype=np.float64)
    tr_YYT = np.trace(np.matmul(Y, Y.T))
    scale = mu / tr_YYT
    M = np.eye(Y.shape[1]) + scale * np.matmul(Y.T, Y)
    M_inv = np.linalg.inv(M)
    B = np.matmul(X, np.matmul(M_inv, X.T))
    B_inv = np.linalg.inv(B)
    w_1 = np.matmul(np.matmul(M_inv, X.T), B_inv)
    w_2 = M_inv - np.matmul(np.matmul(w_1, X), M_inv)
    w_3 = np.sum(np.matmul(w_2, scale * Y.T), axis=1).reshape([-1, 1])
    w_final = w_3 + np.sum(w_1, axis=1).reshape([-1, 1])
    return w_final.T[0]


def _stack(dicts: Sequence[Mapping], streams, splits) -> Dict:
    """target_clip.py:186-190 / :233-242: per (stream, split) the list of feature vectors, in list order."""
    out = {st: {sp: [] for sp in splits} for st in streams}
    for fd in dicts:
        for st, split_features in fd.items():
            for sp, feature in split_features.items():
                out[st][sp].append(feature)
    return out


def dynamic_target_adjustment(valid: List[Mapping], invalid: List[Mapping], splits, streams, b_fraction, replacement: bool,
                              mu: float) -> Dict:
    """target_clip.py:84-104 (+ :161-198, :200-261): one new target {stream: {split: ndarray}}; draws from ``random``
    in the reference's order."""
    if invalid:
        valid = [valid[i] for i in random_fraction(len(valid), b_fraction, replacement)]
        invalid = [invalid[i] for i in random_fraction(len(invalid), b_fraction, replacement)]
        xf, yf = _stack(valid, streams, splits), _stack(invalid, streams, splits)
        return {st: {sp: bootstrap_valid_invalid(xf[st][sp], yf[st][sp], mu) for sp in splits} for st in streams}
    if b_fraction != 1 or replacement is True:
        valid = [valid[i] for i in random_fraction(len(valid), b_fraction, replacement)]
    xf = _stack(valid, streams, splits)
    return {st: {sp: bootstrap_valid(xf[st][sp]) for sp in splits} for st in streams}


def target_features(valid: List[Mapping], invalid: List[Mapping], splits, streams, bootstrap_type: str, mu: float,
                    f_bootstrap, f_memory: float, nbags: int, previous=None) -> Dict:
    """target_clip.py:41-73, cases 3-5 (the caller handles cases 1-2: no bootstrapping -> scaled reference clip)."""
    if bootstrap_type == "simple":
        t = dynamic_target_adjustment(valid, invalid, splits, streams, f_bootstrap, False, mu)
        return {st: {sp: t[st][sp] for sp in splits} for st in streams}
    if bootstrap_type == "partial_update":
        t = dynamic_target_adjustment(valid, invalid, splits, streams, f_bootstrap, False, mu)
        if previous:                                                                     # :75-82
            for st in streams:
                for sp in splits:
                    t[st][sp] = np.multiply(f_memory, t[st][sp]) + np.multiply((1 - f_memory), previous[st][sp])
        return t
    if bootstrap_type == "bagging":                                                      # :145-159
        bags = [dynamic_target_adjustment(valid, invalid, splits, streams, 1, True, mu) for _ in range(nbags)]
        return {st: {sp: np.average([bags[b][st][sp] for b in range(nbags)], axis=0) for sp in splits} for st in streams}
    raise Exception("Error: bootstrap_type should be one of 'simple', 'partial_update', or 'bagging'")


def woodbury_coefficients(G: np.ndarray, m: int, mu: float):
    """The product's route (csrc/vq_boot.hip), in numpy: from the Gram matrix G of the rows [X; Y] (m valid first)
    the coefficients (a, b) with  w = X^T a + Y^T b.  Algebraically equal to bootstrap_valid_invalid / bootstrap_valid:
        scale = mu / tr(Gyy);  K' = (I + scale Gyy)^-1;  C = scale K' Gyx;  gamma = scale K' 1
        B = Gxx - Gxy C;  beta = B^-1 1;  delta = B^-1 Gxy gamma;  a = beta - delta;  b = gamma - C a
    """
    G = np.asarray(G, dtype=np.float64)
    r = G.shape[0]
    n = r - m
    Gxx, Gxy, Gyy = G[:m, :m], G[:m, m:], G[m:, m:]
    scale = mu / np.trace(Gyy) if n > 0 and mu != 0 else 0.0
    if n == 0 or scale == 0.0:
        return np.linalg.solve(Gxx, np.ones(m)), np.zeros(n)
    Kc = np.linalg.solve(np.eye(n) + scale * Gyy, np.concatenate([Gxy.T, np.ones((n, 1))], axis=1))
    C, gamma = scale * Kc[:, :m], scale * Kc[:, m]
    B = Gxx - Gxy @ C
    sol = np.linalg.solve(B, np.stack([np.ones(m), Gxy @ gamma], axis=1))
    a = sol[:, 0] - sol[:, 1]
    return a, gamma - C @ a


def woodbury_target(X_rows: np.ndarray, Y_rows, mu: float) -> np.ndarray:
    """``woodbury_coefficients`` applied: G by BLAS, the solves by LAPACK, w = X^T a + Y^T b."""
    X = np.asarray(X_rows, dtype=np.float64)
    Y = np.zeros((0, X.shape[1])) if Y_rows is None else np.asarray(Y_rows, dtype=np.float64).reshape(-1, X.shape[1])
    R = np.concatenate([X, Y], axis=0)
    a, b = woodbury_coefficients(R @ R.T, X.shape[0], mu)
    return X.T @ a + Y.T @ b


# ---------------------------------------------------------------------------------------------------------------------
# Exact rational references (stdlib ``fractions``).  Every stored value (fp16 / fp32 / fp64) is a dyadic rational, so
# the closed forms are rational functions of exact inputs; they are evaluated without any rounding and the result is
# rounded ONCE to fp64 (int / int true division is correctly rounded).
# ---------------------------------------------------------------------------------------------------------------------
def _exact_int_rows(*blocks):
    """The blocks' values as Python integers over one common power of two: (list of int matrices, e) with value = int * 2^e."""
    mant, expo = [], []
    for blk in blocks:
        a = np.asarray(blk, dtype=np.float64)
        if not np.isfinite(a).all():
            raise ValueError("exact arithmetic needs finite values")
        m, e = np.frexp(a)
        mant.append(m)
        expo.append(e)
    nz = [e[m != 0] for m, e in zip(mant, expo)]
    lo = min([int(v.min()) for v in nz if v.size] or [0]) - 53
    out = []
    for m, e in zip(mant, expo):
        rows = []
        for mr, er in zip(m.reshape(-1, m.shape[-1]), e.reshape(-1, m.shape[-1])):
            rows.append([int(math.ldexp(float(mv), 53)) << (int(ev) - 53 - lo) if mv != 0 else 0 for mv, ev in zip(mr, er)])
        out.append(rows)
    return out, lo


def _frac_solve(A, R):
    """A Z = R over the rationals (lists of lists of Fraction): Gauss-Jordan, first non-zero pivot.  ZeroDivisionError when A is
    singular."""
    dim, nrhs = len(A), len(R[0])
    aug = [list(A[i]) + list(R[i]) for i in range(dim)]
    for k in range(dim):
        p = next((r for r in range(k, dim) if aug[r][k] != 0), None)
        if p is None:
            raise ZeroDivisionError("singular system")
        aug[k], aug[p] = aug[p], aug[k]
        inv = 1 / aug[k][k]
        aug[k] = [v * inv for v in aug[k]]
        for r in range(dim):
            if r != k and aug[r][k] != 0:
                f = aug[r][k]
                rowk = aug[k]
                aug[r] = [v - f * u for v, u in zip(aug[r], rowk)]
    return [row[dim:] for row in aug]


def _round_once(num_over_den_list):
    return np.array([v.numerator / v.denominator for v in num_over_den_list], dtype=np.float64)


def exact_target(X_rows, Y_rows, mu: float) -> np.ndarray:
    """Either closed form of target_clip.py (:192-197 when there is no Y or mu == 0, else :245-260) in exact rational arithmetic
    through the Gram form (the header of csrc/vq_boot.hip), rounded once to fp64.  The Gram matrix is computed in integers.
    Inputs: the values as stored, widened exactly.  ``ZeroDivisionError`` for a singular system or tr(Y Y^T) = 0 with mu != 0."""
    X = np.asarray(X_rows, dtype=np.float64)
    D = X.shape[1]
    Y = np.zeros((0, D)) if Y_rows is None else np.asarray(Y_rows, dtype=np.float64).reshape(-1, D)
    m, n = X.shape[0], Y.shape[0]
    (xi, yi), e = _exact_int_rows(X, Y)
    rows = xi + yi
    r = m + n
    G = [[0] * r for _ in range(r)]                           # integers; the Gram matrix is G * 4^e
    for i in range(r):
        for j in range(i, r):
            G[i][j] = G[j][i] = sum(a * b for a, b in zip(rows[i], rows[j]))
    one = Fraction(1)
    Gxx = [[Fraction(G[i][j]) for j in range(m)] for i in range(m)]
    mu_q = Fraction(float(mu))
    if n == 0 or mu_q == 0:
        a = [z[0] for z in _frac_solve(Gxx, [[one] for _ in range(m)])]
        b = [Fraction(0)] * n
        # solved on the integer matrix (the true one / 4^e): the true a is 4^-e a, and w = (2^e xi)^T 4^-e a = 2^-e xi^T a
        unit = Fraction(2) ** (-e)
    else:
        # in integer units (G = Gram / 4^e):  s Gram = s' G with s' = mu / tr(G);  K = I + s' Gyy
        tr = sum(G[m + j][m + j] for j in range(n))
        s = mu_q / tr                                         # ZeroDivisionError: all-zero Y
        K = [[(one if i == j else 0) + s * G[m + i][m + j] for j in range(n)] for i in range(n)]
        q4 = Fraction(4) ** e                                 # Gyx in true units = G * 4^e; keep true units from here on
        rhs = [[q4 * G[m + i][c] for c in range(m)] + [one] for i in range(n)]
        Z = _frac_solve(K, rhs)                               # K' Gyx | K' 1
        st = s / q4                                           # the true scale  mu / tr(Y Y^T)
        Cm = [[st * Z[j][c] for c in range(m)] for j in range(n)]
        gamma = [st * Z[j][m] for j in range(n)]
        B = [[q4 * G[i][c] - sum(q4 * G[i][m + j] * Cm[j][c] for j in range(n)) for c in range(m)] for i in range(m)]
        rhs2 = [[one, sum(q4 * G[i][m + j] * gamma[j] for j in range(n))] for i in range(m)]
        sol = _frac_solve(B, rhs2)
        a = [z[0] - z[1] for z in sol]
        b = [gamma[j] - sum(Cm[j][i] * a[i] for i in range(m)) for j in range(n)]
        unit = Fraction(2) ** e                               # a, b in true units: w = 2^e * rows_int^T coef
    coef = a + b
    # common denominator -> one integer dot product per element
    den = 1
    for c in coef:
        den = den * c.denominator // math.gcd(den, c.denominator)
    num = [c.numerator * (den // c.denominator) for c in coef]
    scale = unit / den
    w = [Fraction(sum(nk * rows[k][d] for k, nk in enumerate(num))) * scale for d in range(D)]
    return _round_once(w)


def exact_target_explicit(X_rows, Y_rows, mu: float) -> np.ndarray:
    """The reference's own formulas with their explicit inverses (``bootstrap_valid`` / ``bootstrap_valid_invalid`` above, D x D
    for the second), evaluated exactly and rounded once.  O(D^3) rational operations: for small D only."""
    X = [[Fraction(float(v)) for v in row] for row in np.asarray(X_rows, dtype=np.float64)]
    m, D = len(X), len(X[0])
    Y = [] if Y_rows is None else [[Fraction(float(v)) for v in row] for row in np.asarray(Y_rows, dtype=np.float64).reshape(-1, D)]
    n = len(Y)
    one, zero = Fraction(1), Fraction(0)

    def eye(k):
        return [[one if i == j else zero for j in range(k)] for i in range(k)]

    def mm(A, B):
        Bt = list(zip(*B))
        return [[sum(a * b for a, b in zip(ra, cb)) for cb in Bt] for ra in A]

    def tr(A):
        return [list(c) for c in zip(*A)]

    if n == 0:                                                # :192-197  w = X (X^T X)^-1 1 with X = rows^T
        M_inv = _frac_solve(mm(X, tr(X)), eye(m))
        mu_v = [[sum(row)] for row in M_inv]
        return _round_once([v[0] for v in mm(tr(X), mu_v)])
    scale = Fraction(float(mu)) / sum(v * v for row in Y for v in row)            # :248-249
    YtY = mm(tr(Y), Y)
    M = [[(one if i == j else zero) + scale * YtY[i][j] for j in range(D)] for i in range(D)]
    M_inv = _frac_solve(M, eye(D))
    MiXt = mm(M_inv, tr(X))
    B_inv = _frac_solve(mm(X, MiXt), eye(m))
    w_1 = mm(MiXt, B_inv)                                     # [D][m]
    w_1XMi = mm(mm(w_1, X), M_inv)
    w_2 = [[M_inv[i][j] - w_1XMi[i][j] for j in range(D)] for i in range(D)]
    sYt = [[scale * v for v in row] for row in tr(Y)]         # [D][n]
    w_3 = [sum(row) for row in mm(w_2, sYt)]
    return _round_once([w_3[i] + sum(w_1[i]) for i in range(D)])


class SingularSystem(ValueError):
    """``kernel_order_target``: the pivot test of csrc/vq_boot.hip refused (status 1 on the device)."""


PIVOT_TOL_PER_ROW = 16 * 2.0 ** -52         # csrc/vq_boot.hip: a pivot below dim * this * (largest entry the column had) is rounding noise


def _kernel_gauss_jordan(aug: np.ndarray, dim: int) -> int:
    """``gauss_jordan`` of csrc/vq_boot.hip on aug [dim][dim + nrhs] in place, operation for operation (products and sums round
    separately: the library is built without contraction).  Returns the number of row swaps."""
    swaps = 0
    a0 = np.abs(aug[:, :dim])
    floor = (PIVOT_TOL_PER_ROW * dim) * np.where(np.isnan(a0), 0.0, a0).max(axis=0) if dim else a0          # per column, before any elimination
    for k in range(dim):
        col = np.abs(aug[k:, k])
        bv, best = col[0], k
        if not np.isnan(bv) and dim - k > 1:
            rest = np.where(np.isnan(col[1:]), -1.0, col[1:])              # v > bv is false for a NaN
            j = int(np.argmax(rest))                                       # the first maximum, like the strict '>' scan
            if rest[j] > bv:
                bv, best = rest[j], k + 1 + j
        if not (bv > floor[k] and bv < 1.0e300):
            raise SingularSystem("pivot %d: |%r|" % (k, float(bv)))
        if best != k:
            aug[[k, best]] = aug[[best, k]]
            swaps += 1
        inv = 1.0 / aug[k, k]
        aug[k] *= inv
        others = np.arange(dim) != k
        aug[others, k + 1:] -= np.outer(aug[others, k], aug[k, k + 1:])
        aug[others, k] = 0.0
    return swaps


def kernel_order_gram(R: np.ndarray) -> np.ndarray:
    """The Gram matrix as the kernel's waves sum it: each of 64 lanes adds its products d = lane, lane + 64, ... in order, then the
    shuffle tree (offsets 32, 16, .., 1)."""
    r, D = R.shape
    pad = (-D) % 64
    Rp = np.concatenate([R, np.zeros((r, pad))], axis=1) if pad else R          # a lane past the tail adds nothing (s + 0 = s)
    G = np.empty((r, r))
    for i in range(r):
        prod = (Rp[i][None, :] * Rp[i:]).reshape(r - i, -1, 64)
        s = np.zeros((r - i, 64))
        for c in range(prod.shape[1]):
            s = s + prod[:, c]
        for o in (32, 16, 8, 4, 2, 1):
            s = s[:, :o] + s[:, o:2 * o]
        G[i, i:] = s[:, 0]
        G[i:, i] = s[:, 0]
    return G


def kernel_order_target(X_rows, Y_rows, mu: float):
    """csrc/vq_boot.hip restated in fp64 numpy, in the kernel's own order of operations: Gram matrix, the scale, Gauss-Jordan with
    partial pivoting on [I + s Gyy | Gyx | 1] and on [B | 1 | Gxy gamma], the coefficients, the combination of the rows.
    Returns (w, swaps_first_solve, swaps_second_solve); the first solve is the one on I + s Gyy (0 swaps when it does not run).
    Raises ``SingularSystem`` where the kernel reports status 1."""
    X = np.asarray(X_rows, dtype=np.float64)
    D = X.shape[1]
    Y = np.zeros((0, D)) if Y_rows is None else np.asarray(Y_rows, dtype=np.float64).reshape(-1, D)
    m, n = X.shape[0], Y.shape[0]
    r = m + n
    R = np.concatenate([X, Y], axis=0)
    with np.errstate(all="ignore"):
        G = kernel_order_gram(R)
        tr = 0.0
        for j in range(n):
            tr += G[m + j, m + j]
        # mu / 0 = inf, as on the device; a non-finite trace -> NaN (never 0, which would mean "no non-matches")
        scale = (float(np.float64(mu) / np.float64(tr)) if tr < 1.0e300 else float("nan")) if (n > 0 and mu != 0.0) else 0.0
        coef = np.zeros(r)
        sw1 = sw2 = 0
        if n > 0 and scale != 0.0:
            A1 = np.empty((n, n + m + 1))
            A1[:, :n] = np.eye(n) + scale * G[m:, m:]
            A1[:, n:n + m] = G[m:, :m]
            A1[:, n + m] = 1.0
            sw1 = _kernel_gauss_jordan(A1, n)
            T = scale * A1[:, n:]                                          # [n][m + 1]: C | gamma
            S = np.zeros((m, m + 1))
            for j in range(n):
                S = S + np.outer(G[:m, m + j], T[j])
            Bm = np.empty((m, m + 2))
            Bm[:, :m] = G[:m, :m] - S[:, :m]
            Bm[:, m] = 1.0
            Bm[:, m + 1] = S[:, m]
            sw2 = _kernel_gauss_jordan(Bm, m)
            a = Bm[:, m] - Bm[:, m + 1]
            s = np.zeros(n)
            for i in range(m):
                s = s + T[:, i] * a[i]
            coef[:m], coef[m:] = a, T[:, m] - s
        else:
            Bm = np.empty((m, m + 2))
            Bm[:, :m] = G[:m, :m]
            Bm[:, m] = 1.0
            Bm[:, m + 1] = 0.0
            sw2 = _kernel_gauss_jordan(Bm, m)
            coef[:m] = Bm[:, m]
        w = np.zeros(D)
        for k in range(r):
            w = w + coef[k] * R[k]
    return w, sw1, sw2
