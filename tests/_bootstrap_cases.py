"""Inputs and CPU references of the bootstrap edge tests (tests/test_bootstrap_edges_oracle.py proves on the CPU what the table
promises, tests/test_bootstrap_edges_gpu.py runs csrc/vq_boot.hip on it).  No product code here.

A case is (m validated matches, n validated non-matches, D, spread, mu).  Its rows are |N(0,1)| values times a per-row factor
10^U(-spread, spread), seeded by the shape, cast to the storage type and widened again: every reference sees exactly the values
the device sees.  Row norms that differ by orders of magnitude are what makes partial pivoting swap rows often, in either solve, and
with right-hand sides that differ (rows of similar norm rarely do: the recorded fixtures swap twice in the second solve, never in
the first; independent rows of equal scale not at all).

References, each computed once per process:
  exact     oracle.exact_target: the closed form in rational arithmetic, rounded once (cases up to 20 rows)
  kernel    oracle.kernel_order_target: the kernel's own sequence in fp64 numpy, with the row swaps of either solve counted
  woodbury  oracle.woodbury_target: BLAS Gram matrix + LAPACK solves
  explicit  oracle.bootstrap_valid[_invalid]: the reference's explicit inverses (D x D for the second form)
and the case's ``spread``: how far these roundings of one formula lie apart, relative to max|w| (see ``references``).
"""
import functools
from collections import namedtuple

import numpy as np

import bootstrap_oracle as bo

Case = namedtuple("Case", "m n D spread mu")

# purpose -> cases; the smallest shapes that reach each path of the kernel
TAILS = [Case(3, 2, 4, 1.5, 0.3), Case(6, 4, 64, 1.5, 0.3), Case(6, 4, 68, 1.5, 0.3), Case(12, 8, 100, 1.5, 0.3),
         Case(12, 8, 260, 1.5, 0.3)]                                   # D below / at / past the 64-lane stride, past the 256-thread stride
SWAPS_SECOND = [Case(9, 0, 260, 2, 0.0), Case(12, 8, 260, 2, 1.5)]     # the solve on Gxx / on B
SWAPS_FIRST = [Case(6, 10, 64, 1.5, 40.0), Case(6, 10, 64, 1.5, 400.0)]    # the solve on I + s Gyy swaps only when mu is large
SINGLE = [Case(1, 0, 64, 1.5, 0.3), Case(1, 1, 64, 1.5, 0.3), Case(1, 19, 68, 1, 0.3)]
EXACT = TAILS + SWAPS_SECOND + SWAPS_FIRST + SINGLE
FULL = [Case(256, 0, 1024, 1, 0.0), Case(128, 128, 1024, 1, 0.3), Case(1, 255, 1024, 1, 0.3), Case(255, 1, 1024, 0, 1.5),
        Case(100, 156, 260, 1, 0.3)]                                   # m + n = BOOT_MAX_ROWS
WIDE = [Case(5, 3, 2048, 1, 0.3)]
LARGE = FULL + WIDE
ALL = EXACT + LARGE
MARGIN = 8                 # device within MARGIN * spread * max|w_ref|: the device is one more rounding of the same formula


def case_id(c):
    return "m%d-n%d-D%d-s%g-mu%g" % c


def _seed(c):
    return 1000 * c.m + 10 * c.n + c.D


@functools.lru_cache(maxsize=None)
def rows(c, dtype="float64"):
    """(X [m][D], Y [n][D] or None) of case c in fp64, holding values of ``dtype`` (float16 / float32 / float64) exactly."""
    rng = np.random.default_rng(_seed(c))
    r = c.m + c.n
    R = np.abs(rng.standard_normal((r, c.D))) * 10.0 ** rng.uniform(-c.spread, c.spread, (r, 1))
    R = R.astype(np.dtype(dtype)).astype(np.float64)
    assert np.isfinite(R).all()
    R.setflags(write=False)
    return R[:c.m], (R[c.m:] if c.n else None)


def rel(a, b):
    """max|a - b| relative to max|b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


Refs = namedtuple("Refs", "w_ref spread exact kernel woodbury explicit swaps_first swaps_second")


def references_of(X, Y, mu, exact):
    """The references of one problem.  With ``exact``: w_ref is the exact target and spread the largest relative distance of the
    three fp64 routes from it; without: w_ref is the Woodbury route and spread the largest pairwise distance of the three."""
    kern, sw1, sw2 = bo.kernel_order_target(X, Y, mu)
    wood = bo.woodbury_target(X, Y, mu)
    expl = bo.bootstrap_valid(X) if Y is None else bo.bootstrap_valid_invalid(X, Y, mu)
    if exact:
        ex = bo.exact_target(X, Y, mu)
        spread = max(rel(kern, ex), rel(wood, ex), rel(expl, ex))
        w_ref = ex
    else:
        ex = None
        spread = max(rel(kern, wood), rel(expl, wood), rel(wood, kern), rel(expl, kern), rel(kern, expl), rel(wood, expl))
        w_ref = wood
    for a in (w_ref, kern, wood, expl):
        a.setflags(write=False)
    return Refs(w_ref, spread, ex, kern, wood, expl, sw1, sw2)


@functools.lru_cache(maxsize=None)
def references(c, dtype="float64"):
    X, Y = rows(c, dtype)
    return references_of(X, Y, c.mu, c in EXACT)


# ----------------------------------------------------------------------------------------------------------------------------
# resident databases: [N][S][E][D] blocks whose (stream, split) slots are independent problems on the rows below
RES_N = 12
RES_VALID = (0, 3, 7, RES_N - 1)           # rows 0 and n - 1 included
RES_INVALID = (1, 5, 10)
RES_MU = 0.3
RES_SPREAD = 1.0


@functools.lru_cache(maxsize=None)
def resident_block(S, E, D, dtype):
    """[RES_N][S][E][D] in ``dtype``: |N(0,1)| times a per-(row, slot) factor 10^U(-1, 1).  float16: the values ARE halves."""
    rng = np.random.default_rng(7000 + 100 * S + 10 * E + D)
    x = np.abs(rng.standard_normal((RES_N, S, E, D))) * 10.0 ** rng.uniform(-RES_SPREAD, RES_SPREAD, (RES_N, S, E, 1))
    x = x.astype(np.dtype(dtype))
    assert np.isfinite(x).all()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def resident_references(S, E, D, dtype, with_invalid=True):
    """[S][E] Refs (exact: 7 rows) of the problems ``bootstrap_target(RES_VALID, RES_INVALID, RES_MU)`` poses."""
    x = resident_block(S, E, D, dtype).astype(np.float64)
    out = [[None] * E for _ in range(S)]
    for s in range(S):
        for e in range(E):
            X = x[list(RES_VALID), s, e]
            Y = x[list(RES_INVALID), s, e] if with_invalid else None
            out[s][e] = references_of(X, Y, RES_MU if with_invalid else 0.0, True)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# Linearly dependent inputs.  Each was picked (on the CPU, in kernel order) among those whose elimination leaves a NON-ZERO residue
# where the dependent row's pivot should vanish: a pivot test "> 0" accepts them and returns a finite target.
DEPENDENT = Case(6, 4, 68, 1.0, 0.3)
RES_TWICE = {"float16": ([0, 0, 3, 7, 11], 0.0), "float32": ([0, 3, 11, 7, 11], 0.0), "float64": ([0, 3, 7, 7, 11], 0.3)}   # valid rows, mu


def dependent_host(kind):
    """(X, Y or None, mu) in fp64: row 4 of DEPENDENT once more ("duplicate") or doubled ("double"), no non-matches."""
    X, _ = rows(DEPENDENT)
    return np.insert(X, 4, {"duplicate": 1.0, "double": 2.0}[kind] * X[4], axis=0), None, 0.0


# ----------------------------------------------------------------------------------------------------------------------------
def scaled_query_exact(r):
    """target_clip.py:311-313, t = r / (r . r), with the products and their sum exact (what math.fsum stands for) and one rounding
    at the end."""
    from fractions import Fraction
    q = [Fraction(float(v)) for v in r]
    rr = sum(v * v for v in q)
    return np.array([(v / rr).numerator / (v / rr).denominator for v in q], dtype=np.float64)


def ragged_launch(P=54, D=1024, seed=54):
    """P problems of one launch, sizes shuffled: the 256-row problem Case(128, 128, 1024, 1, 0.3) beside 1-row problems and small
    ragged ones.  Returns [(X, Y or None)] in launch order (fp64)."""
    rng = np.random.default_rng(seed)
    big = Case(128, 128, D, 1, 0.3)
    sizes = [(1, 0)] * 6 + [(1, 1)] * 3 + [(1, 7), (2, 0), (7, 1)]
    while len(sizes) < P - 1:
        sizes.append((int(rng.integers(1, 13)), int(rng.integers(0, 10))))
    probs = [rows(big)]
    for m, n in sizes:
        R = np.abs(rng.standard_normal((m + n, D))) * 10.0 ** rng.uniform(-1, 1, (m + n, 1))
        probs.append((R[:m], R[m:] if n else None))
    order = rng.permutation(P)
    return [probs[i] for i in order]
