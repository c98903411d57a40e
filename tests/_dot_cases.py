"""Test infrastructure for the dot products in front of the ranking kernels (csrc/vq_sim.hip, csrc/vq_sim_batch.hip: scan_kernel, scan_tiled_kernel,
scan_generic_kernel, batch_fused_kernel, batch_view_kernel): hard feature vectors with an EXACT reference and a DERIVED tolerance.
tests/test_dot_cases.py checks this table on the CPU, tests/test_dot_hard_gpu.py and tests/_dot_hard_child.py run the kernels on it.

Exactness.  Every vector is built in its storage type (float16: 11 significant bits, float32: 24, float64: float32 values stored as
doubles, 24) and every query value carries at most 29 significant bits, so every product x_k t_k has at most 53 and is exactly
representable in binary64 (no product leaves the normal range: the query scales below see to that).  ``math.fsum`` of the products
is then the correctly rounded exact dot ``ref``; ``mag`` = fsum(|x_k t_k|).

Tolerance.  Any order of binary64 additions or FMAs over D exact products obeys |got - ref| <= (D-1)u/(1-(D-1)u) mag, u = 2^-53; the
tests use D 2^-53 mag per dot (``dot_bound``).  A stream mean over the m splits present is m - 1 additions and a division: m
roundings of a value no larger than sum|sim_e| / m on the device and as many in the reference's own sequential rule, so
``sum of the dot bounds + (m + 1) 2^-53 sum|sim_e|`` holds both (``avg_bound``; m = 1: the division by one is exact).

Groups.  One query serves all rows of a database, and no single query scale suits every family in every type (float64 rows within a
factor two of the largest finite value overflow under the query that brings float32 subnormals to O(1)).  So a table is one of three
GROUPS, each a database with its own query: ``plain`` (signs, cancel, range, zeros, nonfinite), ``sub`` (subnormal) and ``ext``
(extreme).  In every database the even rows are ``signs`` fillers (at the group's scale) and the odd rows walk the group's other
families, so neighbouring rows never share a family, and a non-finite row never sits in column 15 of its 16-row tile: both its
neighbours inside the tile are finite.  n % 16 == 5 in every group.

The query of slot (s, e): D / 2 values of 29 significant bits, each at TWO positions (a seeded perfect matching), with random sign;
in ``plain`` the exponent of pair j walks 24 binades (g_j from -12 to 12).  ``cancel`` rows put (a, -a) on a pair, ``range`` rows
carry the inverse exponents.  Pair 0 is special: positive, g = -12, and the query is exactly 0 at its second position (the class
"inf against a query element of exactly 0")."""
import math

import numpy as np

U = 2.0 ** -53
DTYPES = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
SIG_BITS = {"f16": 11, "f32": 24, "f64": 24}
EMAX = {"f16": 15, "f32": 127, "f64": 1023}
GROUPS = ("plain", "sub", "ext")
GROUP_N = {"plain": 197, "sub": 37, "ext": 37}
GROUP_FAMILIES = {"plain": ("signs", "cancel", "range", "zeros", "nonfinite"), "sub": ("signs", "subnormal"), "ext": ("signs", "extreme")}
FAMILIES = ("signs", "cancel", "subnormal", "extreme", "range", "zeros", "nonfinite")
NONFINITE = ("pos_inf", "inf_minus_inf", "nan", "inf_times_zero")
SPREAD = 12                                                    # plain: g_j in [-SPREAD, SPREAD]
WEIGHTS = [1.0, 1.5, 0.75]


def query_exponent(group, dtype_name):
    """The power of two that scales the group's query: plain 2^-5 (D products of ordinary size sum to O(1)); sub brings the type's
    subnormals (float64: float32's) to products of about 2^-5; ext takes values near the largest finite one down to about 2^4."""
    if group == "plain":
        return -5
    if group == "sub":
        return 9 if dtype_name == "f16" else 121
    return -(EMAX[dtype_name] - 3)


def filler_exponent(group, dtype_name):
    """``signs`` rows of a group: ordinary size, but large in ``ext`` (float64: a product with the 2^-1020 query must stay normal)."""
    return EMAX[dtype_name] - 8 if group == "ext" else 0


def slot_layout(D, v, seed):
    """(perm, g, sign) of slot v: pair j = positions perm[2j], perm[2j+1]; g[j] its exponent offset (plain), sign[j] = +-1"""
    rng = np.random.default_rng([seed, D, v, 1])
    perm = rng.permutation(D)
    npairs = D // 2
    g = np.round(np.linspace(-SPREAD, SPREAD, npairs)).astype(np.int64)
    sign = np.where(rng.random(npairs) < 0.5, -1.0, 1.0)
    sign[:min(3, npairs)] = 1.0                                # the non-finite classes need positive query values to aim at
    return perm, g, sign


def make_query(group, dtype_name, S, E, D, seed=0):
    """t [S,E,D] float64, 29 significant bits per value"""
    assert D % 4 == 0
    t = np.zeros((S * E, D))
    for v in range(S * E):
        perm, g, sign = slot_layout(D, v, seed)
        rng = np.random.default_rng([seed, D, v, 2])
        sig = rng.integers(1 << 28, 1 << 29, D // 2).astype(np.float64) * 2.0 ** -28
        val = sign * sig * 2.0 ** (query_exponent(group, dtype_name) + (g if group == "plain" else 0))
        t[v, perm[0::2]] = val
        t[v, perm[1::2]] = val
        t[v, perm[1]] = 0.0
    return t.reshape(S, E, D)


def query_variant(table, q):
    """Query q of a batched pass: the table's query times +1, -1, +2, -1/2 (q mod 4; every product stays exact and normal), and for
    q mod 4 == 2 exactly 0 where the ``pos_inf`` row has its infinity -- the same clip is +inf under query 0, -inf under query 1
    and NaN under query 2, next to each other in one block of the matrix pass."""
    t = table.t * (1.0, -1.0, 2.0, -0.5)[q % 4]
    if q % 4 == 2:
        for v, k in table.inf_pos.items():
            t.reshape(-1, table.D)[v, k] = 0.0
    return t


def _sig(rng, bits, size):
    return rng.integers(1 << (bits - 1), 1 << bits, size).astype(np.float64) * 2.0 ** -(bits - 1)


def _signs(rng, bits, D, scale, negative=False):
    x = _sig(rng, bits, D) * 2.0 ** (rng.integers(-2, 2, D) + scale)
    return -x if negative else x * np.where(rng.random(D) < 0.5, -1.0, 1.0)


def make_vector(family, variant, dtype_name, group, D, v, t_v, rng, seed=0):
    """One vector of D float64 values, each exactly representable in the storage type.  Returns (x, note)."""
    bits = SIG_BITS[dtype_name]
    perm, g, _sign = slot_layout(D, v, seed)
    fill = filler_exponent(group, dtype_name)
    if family == "signs":
        return _signs(rng, bits, D, fill, negative=(variant == "negative")), None
    if family == "cancel":
        x = np.zeros(D)
        a = _sig(rng, bits, D // 2) * 2.0 ** (-g)
        flip = np.where(rng.random(D // 2) < 0.5, -1.0, 1.0)
        x[perm[0::2]] = a * flip
        x[perm[1::2]] = -a * flip
        x[perm[0]] = x[perm[1]] = 0.0
        mag = float(np.abs(x * t_v).sum())
        x[perm[0]] = 2.0 ** round(math.log2(mag * 2.0 ** -24 / abs(t_v[perm[0]])))      # the residual: one power of two
        return x, None
    if family == "range":
        gk = np.empty(D, dtype=np.int64)
        gk[perm[0::2]] = g
        gk[perm[1::2]] = g
        return _sig(rng, bits, D) * 2.0 ** (-gk) * np.where(rng.random(D) < 0.5, -1.0, 1.0), None
    if family == "zeros":
        if variant == "plus":
            return np.zeros(D), None
        if variant == "minus":
            return -np.zeros(D), None
        x = np.zeros(D)
        x[int(variant)] = float(_signs(rng, bits, 1, fill)[0])
        return x, None
    if family == "subnormal":
        if dtype_name == "f16":
            k, unit = rng.integers(1, 1 << 10, D), 2.0 ** -24
        else:
            k, unit = rng.integers(1, 1 << 23, D), 2.0 ** -149
        return k.astype(np.float64) * unit * np.where(rng.random(D) < 0.5, -1.0, 1.0), None
    if family == "extreme":
        return _sig(rng, bits, D) * 2.0 ** EMAX[dtype_name] * np.where(rng.random(D) < 0.5, -1.0, 1.0), None
    assert family == "nonfinite"
    x = _signs(rng, bits, D, fill)
    pos = [int(k) for k in perm if t_v[k] > 0]                 # pair 0's first position and pairs 1 and 2 are positive
    if variant == "pos_inf":
        x[pos[0]] = np.inf
        return x, pos[0]
    if variant == "inf_minus_inf":
        x[pos[0]], x[pos[1]] = np.inf, -np.inf
    elif variant == "nan":
        x[pos[1]] = np.nan
    else:
        x[perm[1]] = np.inf                                    # the query is exactly 0 there
    return x, None


def zero_positions(D):
    return sorted({k for k in (0, 3, 4, 255, 256, D - 4, D - 1) if 0 <= k < D})


class Table:
    """A database of hard rows and its query.  x [n,S,E,D] in the storage type, t [S,E,D]; family / variant per row; ``bad_split``:
    the split of every stream that holds a non-finite row's non-finite value (its other splits are finite);
    ``inf_pos``: slot -> position of the infinity of the ``pos_inf`` row."""

    def __init__(self, group, dtype_name, S, E, D, seed=0):
        self.group, self.dtype_name, self.dtype, self.S, self.E, self.D, self.seed = group, dtype_name, DTYPES[dtype_name], S, E, D, seed
        self.n = n = GROUP_N[group]
        assert n % 16 == 5
        self.t = make_query(group, dtype_name, S, E, D, seed)
        self.bad_split = E - 1
        hard = []
        for fam in GROUP_FAMILIES[group][1:]:
            if fam == "zeros":
                hard += [(fam, var) for var in ["plus", "minus"] + [str(k) for k in zero_positions(D)]]
            elif fam == "nonfinite":
                hard += [(fam, var) for var in NONFINITE]
            else:
                hard += [(fam, "a"), (fam, "b")]
        # odd rows: the hard rows once each, family by family in turn, then more of the seeded families; even rows: signs
        by_family = {}
        for h in hard:
            by_family.setdefault(h[0], []).append(h)
        once = []
        while any(by_family.values()):
            for fam in list(by_family):
                if by_family[fam]:
                    once.append(by_family[fam].pop(0))
        seeded = [f for f in GROUP_FAMILIES[group][1:] if f not in ("zeros", "nonfinite")]
        self.family, self.variant = [], []
        extra = 0
        for r in range(n):
            if r % 2 == 0:
                fam, var = "signs", ("negative" if r % 8 == 0 else "mixed")
            elif once and not (once[0][0] == "nonfinite" and r % 16 == 15):
                fam, var = once.pop(0)
            else:
                fam, var = seeded[extra % len(seeded)], "x%d" % extra
                extra += 1
            self.family.append(fam)
            self.variant.append(var)
        assert not once
        self.family = np.array(self.family)
        x = np.zeros((n, S * E, D))
        self.inf_pos = {}
        tv = self.t.reshape(S * E, D)
        for r in range(n):
            for v in range(S * E):
                rng = np.random.default_rng([seed, D, v, 3, r])
                fam, var = self.family[r], self.variant[r]
                if fam == "nonfinite" and v % E != self.bad_split:
                    fam, var = "signs", "mixed"                # the other splits of a non-finite row are finite
                x[r, v], note = make_vector(fam, var, dtype_name, group, D, v, tv[v], rng, seed)
                if note is not None:
                    self.inf_pos[v] = note
        with np.errstate(over="raise"):
            self.x = x.reshape(n, S, E, D).astype(self.dtype)
        self.x64 = x.reshape(n, S, E, D)
        self.nonfinite_rows = np.flatnonzero(self.family == "nonfinite")

    def rows_of(self, family):
        return np.flatnonzero(self.family == family)

    def expected(self, masked=False, q=0):
        """Expected results under query variant q (0: the table's own query), with or without the mask; computed once"""
        cache = self.__dict__.setdefault("_expected", {})
        if ("dots", q % 4) not in cache:
            cache[("dots", q % 4)] = exact_dots(self.x, query_variant(self, q))
        if (masked, q % 4) not in cache:
            cache[(masked, q % 4)] = Expected(self.x, None, self.mask() if masked else None, dots=cache[("dots", q % 4)])
        return cache[(masked, q % 4)]

    def mask(self):
        """Presence mask [n,S,E]: about 80 % present; every non-finite split absent and the finite splits of those rows present;
        row 2 lacks stream 0 altogether and the last row every split of the last stream."""
        p = (np.random.default_rng([self.seed, 5, self.n, self.S, self.E]).random((self.n, self.S, self.E)) < 0.8).astype(np.uint8)
        p[self.nonfinite_rows] = 1
        p[self.nonfinite_rows, :, self.bad_split] = 0
        p[2, 0, :] = 0
        p[self.n - 1, self.S - 1, :] = 0
        return p

    def view_rows(self):
        """Rows of a view: drops the row BEFORE every non-finite row and some others; keeps every hard row and the last row"""
        keep = np.random.default_rng([self.seed, 6, self.n]).random(self.n) < 0.6
        keep[self.family != "signs"] = True
        keep[self.nonfinite_rows - 1] = False
        keep[self.n - 1] = True
        return np.flatnonzero(keep).astype(np.int64)

    def tile_view_rows(self):
        """The same for a tiled database, with tiles touched in one clip only (beyond the non-finite rows, which all stay) and, in the
        plain group, one not touched at all"""
        keep = np.zeros(self.n, dtype=bool)
        keep[self.view_rows()] = True
        for tile, col in (((5, 3), (8, 9)) if self.n > 160 else ((1, 3),)):
            keep[16 * tile:16 * tile + 16] = False
            keep[16 * tile + col] = True
        if self.n > 176:
            keep[160:176] = False
        assert keep[self.nonfinite_rows].all() and (np.bincount(np.flatnonzero(keep) >> 4) == 1).any()
        return np.flatnonzero(keep).astype(np.int64)


_tables = {}


def table(group, dtype_name, S, E, D, seed=0):
    key = (group, dtype_name, S, E, D, seed)
    if key not in _tables:
        _tables[key] = Table(*key)
    return _tables[key]


# --------------------------------------------------------------------------------------------------------------------- the reference
def exact_dots(x, t):
    """x [n,S,E,D] (any float type), t [S,E,D] -> (ref, mag) [n,S,E]: the correctly rounded exact dot of every vector and the sum of
    the absolute products; a vector with a non-finite product gets its class as the value (+-inf, or NaN: a NaN product, products of
    both infinities, inf times 0) and mag = inf."""
    n, S, E, D = x.shape
    with np.errstate(invalid="ignore", over="raise"):
        p = x.astype(np.float64) * np.asarray(t, dtype=np.float64)[None]
    ref, mag = np.empty((n, S, E)), np.empty((n, S, E))
    fin = np.isfinite(p).all(axis=3)
    for idx in np.ndindex(n, S, E):
        if fin[idx]:
            row = p[idx].tolist()
            ref[idx], mag[idx] = math.fsum(row), math.fsum(map(abs, row))
        else:
            row = p[idx]
            mag[idx] = np.inf
            if np.isnan(row).any() or ((row == np.inf).any() and (row == -np.inf).any()):
                ref[idx] = np.nan
            else:
                ref[idx] = np.inf if (row == np.inf).any() else -np.inf
    return ref, mag


def dot_bound(mag, D):
    return D * U * mag


def reference_avg(ref, present=None):
    """The reference's rule (oracle/sim_oracle.py dense_similarities): the sequential sum over the splits present, divided by their
    count; NaN where none is.  -> (avg [n,S], n_e [n,S] int32)"""
    n, S, E = ref.shape
    pres = np.ones((n, S, E), dtype=bool) if present is None else np.asarray(present).astype(bool)
    acc = np.zeros((n, S))
    with np.errstate(invalid="ignore", divide="ignore"):
        for e in range(E):
            acc = np.where(pres[:, :, e], acc + ref[:, :, e], acc)
        n_e = pres.sum(axis=2).astype(np.int32)
        return acc / n_e, n_e


def avg_bound(ref, mag, D, present=None):
    """[n,S]: sum of the dot bounds of the splits present + (m + 1) 2^-53 sum |sim_e|; inf where a present split is not finite"""
    pres = np.ones(ref.shape, dtype=bool) if present is None else np.asarray(present).astype(bool)
    m = pres.sum(axis=2)
    with np.errstate(invalid="ignore"):
        return np.where(pres, dot_bound(mag, D), 0.0).sum(axis=2) + (m + 1) * U * np.where(pres, np.abs(ref), 0.0).sum(axis=2)


class Expected:
    """What a scan of (x, t) under ``present`` must return."""

    def __init__(self, x, t, present=None, dots=None):
        self.D = x.shape[3]
        self.ref, self.mag = exact_dots(x, t) if dots is None else dots
        self.present = present
        self.avg, self.n_e = reference_avg(self.ref, present)
        self.avg_bound = avg_bound(self.ref, self.mag, self.D, present)
        self.sim_bound = dot_bound(self.mag, self.D)


def same_class(got, want):
    """element-wise: NaN where NaN is wanted, the same infinity where one is wanted (only looked at where ``want`` is not finite)"""
    return np.where(np.isnan(want), np.isnan(got), got == want)


def _pairs(exp, avg, sims, rows):
    pairs = [(avg, exp.avg[rows], exp.avg_bound[rows])]
    if sims is not None:
        pairs.append((sims, exp.ref[rows], exp.sim_bound[rows]))
    return pairs


def violations(exp, avg, sims=None, rows=None):
    """bool per row: some avg (or sim) of the row is outside its bound, not finite where it must be, or not of the class due"""
    rows = np.arange(exp.ref.shape[0]) if rows is None else rows
    bad = np.zeros(len(rows), dtype=bool)
    for got, want, bound in _pairs(exp, avg, sims, rows):
        fin = np.isfinite(want)
        with np.errstate(invalid="ignore"):
            ok = np.where(fin, np.isfinite(got) & (np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)) <= np.where(fin, bound, 0.0)),
                          same_class(got, want))
        bad |= ~ok.reshape(len(rows), -1).all(axis=1)
    return bad


def check_against(exp, family, avg, n_e, sims=None, rows=None):
    """Device results against the expectation (at ``rows`` of the table if the results are a view's): n_e exact; every finite sim and
    avg inside its bound, every non-finite one of its class (NaN also where no split is present); nothing else.  Returns
    ({family: worst |err| / bound}, number of finite values checked, number of classes checked)."""
    rows = np.arange(exp.ref.shape[0]) if rows is None else rows
    fam = family[rows]
    assert avg.shape == exp.avg[rows].shape and (n_e == exp.n_e[rows]).all(), "n_e"
    bad = violations(exp, avg, sims, rows)
    assert not bad.any(), "rows %s (%s): outside the bound, or not the class due" % (rows[bad][:8], fam[bad][:8])
    worst, n_fin, n_cls = {}, 0, 0
    for got, want, bound in _pairs(exp, avg, sims, rows):
        fin = np.isfinite(want)
        err = np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0))
        bnd = np.where(fin, bound, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err > 0, err / bnd, 0.0)
        ratio = ratio.reshape(ratio.shape[0], -1).max(axis=1)
        for f in np.unique(fam):
            worst[f] = max(worst.get(f, 0.0), float(ratio[fam == f].max()))
        n_fin += int(fin.sum())
        n_cls += int((~fin).sum())
    return worst, n_fin, n_cls


def ratio_line(worst):
    return " ".join("%s=%.3f" % (f, worst[f]) for f in FAMILIES if f in worst)
