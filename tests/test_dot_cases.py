"""CPU: the hard-vector table of tests/_dot_cases.py is what it says -- exact products, families that meet their conditions, a bound
that three honest binary64 summation orders keep and that deliberately wrong host dots break, each on the family named here.  The
GPU tests (tests/test_dot_hard_gpu.py) apply the same ``check_against`` to what the kernels return."""
from fractions import Fraction

import numpy as np
import pytest

import _dot_cases as dc

SHAPE = (2, 3)
DS = (1024, 260, 4)
TYPES = ("f16", "f32", "f64")
CASES = [(g, d, D) for g in dc.GROUPS for d in TYPES for D in DS]


def products(tb, t=None):
    with np.errstate(invalid="ignore"):
        return tb.x.astype(np.float64) * (tb.t if t is None else t)[None]


# ------------------------------------------------------------------------------------------------------------- host dots, honest and not
def dot_numpy(tb):
    x = tb.x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([[[np.dot(x[r, s, e], tb.t[s, e]) for e in range(tb.E)] for s in range(tb.S)] for r in range(tb.n)])


def dot_sequential(tb, p=None, dtype=np.float64):
    p = products(tb) if p is None else p
    with np.errstate(invalid="ignore", over="ignore"):
        return np.add.accumulate(p.astype(dtype), axis=3, dtype=dtype)[..., -1].astype(np.float64)


def dot_lanes(tb):
    """scan_generic_kernel's order: lane l walks the quads at 4 l + 256 i, then the butterfly over the 64 lanes"""
    p = products(tb)
    pad = (-tb.D) % 256
    p = np.concatenate([p, np.zeros(p.shape[:3] + (pad,))], axis=3)                    # adding an exact zero changes no partial sum
    lanes = p.reshape(p.shape[:3] + (-1, 64, 4)).transpose(0, 1, 2, 4, 3, 5).reshape(p.shape[:3] + (64, -1))
    with np.errstate(invalid="ignore"):
        v = np.add.accumulate(lanes, axis=4)[..., -1]
        for step in (32, 16, 8, 4, 2, 1):
            v = v + v[..., np.arange(64) ^ step]
    return v[..., 0]


def host_results(tb, sims, present=None, skip=True):
    """avg and n_e from sims by the reference's rule -- or, ``skip`` False, with the mask as a factor 0 / 1"""
    if skip:
        avg, n_e = dc.reference_avg(sims, present)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            n_e = present.sum(axis=2).astype(np.int32)
            acc = np.zeros(n_e.shape)
            for e in range(tb.E):
                acc = acc + sims[:, :, e] * present[:, :, e]
            avg = acc / n_e
    return avg, n_e


def rejected_families(tb, exp, sims, present=None, skip=True):
    avg, _ = host_results(tb, sims, present, skip)
    bad = dc.violations(exp, avg, sims)
    return set(tb.family[bad].tolist()), bad


@pytest.fixture(scope="module")
def expected():
    cache = {}

    def get(group, dtype_name, D, masked=False):
        key = (group, dtype_name, D, masked)
        if key not in cache:
            tb = dc.table(group, dtype_name, *SHAPE, D)
            cache[key] = (tb, dc.Expected(tb.x, tb.t, tb.mask() if masked else None))
        return cache[key]
    return get


# ------------------------------------------------------------------------------------------------------------- the table itself
@pytest.mark.parametrize("group,dtype_name,D", CASES)
def test_values_live_in_the_storage_type_and_products_are_exact(expected, group, dtype_name, D):
    tb, exp = expected(group, dtype_name, D)
    assert tb.x.dtype == dc.DTYPES[dtype_name] and tb.n % 16 == 5
    back = tb.x.astype(np.float64)
    assert ((back == tb.x64) | (np.isnan(back) & np.isnan(tb.x64))).all() and (np.signbit(back) == np.signbit(tb.x64)).all()
    if dtype_name == "f64":
        m, _ = np.frexp(back[np.isfinite(back)])
        assert (m * 2.0 ** 24 == np.round(m * 2.0 ** 24)).all(), "24 significant bits in float64 rows"
    m, _ = np.frexp(tb.t)
    assert (m * 2.0 ** 29 == np.round(m * 2.0 ** 29)).all(), "29 significant bits in the query"
    # every element of one vector per family (every variant of zeros and nonfinite) through exact rationals
    seen = set()
    for r in range(tb.n):
        key = (tb.family[r], tb.variant[r] if tb.family[r] in ("zeros", "nonfinite") else "")
        if key in seen:
            continue
        seen.add(key)
        for s, e in np.ndindex(tb.S, tb.E):
            xs, ts = tb.x[r, s, e].astype(np.float64).tolist(), tb.t[s, e].tolist()
            if not np.isfinite(xs).all():
                continue
            exact = [Fraction(a) * Fraction(b) for a, b in zip(xs, ts)]
            assert all(Fraction(a * b) == p for a, b, p in zip(xs, ts, exact)), (tb.family[r], r, s, e)
            assert all(p == 0 or abs(p) >= Fraction(2.0 ** -1022) for p in exact), "a product below the normal range"
            assert float(sum(exact)) == exp.ref[r, s, e] and float(sum(abs(p) for p in exact)) == exp.mag[r, s, e], (tb.family[r], r, s, e)
    assert {k[0] for k in seen} == set(dc.GROUP_FAMILIES[group])


@pytest.mark.parametrize("group,dtype_name,D", CASES)
def test_each_family_meets_its_condition(expected, group, dtype_name, D):
    tb, exp = expected(group, dtype_name, D)
    x = tb.x.astype(np.float64)
    fam = tb.family
    assert (fam[0::2] == "signs").all() and (fam[1::2] != "signs").all(), "neighbouring rows are of different families"
    rows = tb.rows_of("signs")
    neg = [r for r in rows if tb.variant[r] == "negative"]
    assert neg and (x[neg] < 0).all() and all((x[r] < 0).any() and (x[r] > 0).any() for r in rows if tb.variant[r] == "mixed")
    tiny = {"f16": 2.0 ** -14, "f32": 2.0 ** -126, "f64": 2.0 ** -126}[dtype_name]
    if group == "plain":
        c = tb.rows_of("cancel")
        ratio = exp.mag[c] / np.abs(exp.ref[c])
        assert c.size >= 2 and (ratio >= 2.0 ** 20).all() and (exp.sim_bound[c] <= 2.0 ** -10 * np.abs(exp.ref[c])).all(), (ratio.min(), ratio.max())
        rg = tb.rows_of("range")
        _, ex = np.frexp(x[rg])
        _, et = np.frexp(np.where(tb.t == 0, 1.0, tb.t))
        assert rg.size >= 2 and (ex.max(axis=3) - ex.min(axis=3) >= 20).all() and (et.max(axis=2) - et.min(axis=2) >= 20).all()
        _, ep = np.frexp(x[rg] * tb.t)
        live = (tb.t != 0)[None].repeat(rg.size, axis=0)
        assert ep[live].max() - ep[live].min() <= 3, "the query carries the inverse spread"
        z = tb.rows_of("zeros")
        variants = [tb.variant[r] for r in z]
        assert variants[:2] == ["plus", "minus"] and [int(v) for v in variants[2:]] == dc.zero_positions(D)
        assert (x[z[0]] == 0).all() and not np.signbit(x[z[0]]).any() and (x[z[1]] == 0).all() and np.signbit(x[z[1]]).all()
        for r, v in zip(z[2:], variants[2:]):
            assert ((x[r] != 0).sum(axis=2) == 1).all() and (x[r][..., int(v)] != 0).all()
        assert (exp.ref[z[:2]] == 0).all() and (exp.mag[z[:2]] == 0).all()
        nf = tb.nonfinite_rows
        assert [tb.variant[r] for r in nf] == list(dc.NONFINITE) and (nf % 16 != 15).all() and (nf % 16 != 0).all()
        b = tb.bad_split
        assert (exp.ref[nf[0], :, b] == np.inf).all() and np.isnan(exp.ref[nf[1:], :, b]).all()
        assert np.isfinite(np.delete(exp.ref, b, axis=2)).all() and np.isfinite(np.delete(exp.ref, nf, axis=0)).all()
        assert np.isinf(x[nf[3], :, b]).sum() == tb.S and all(tb.t[s, b][np.isinf(x[nf[3], s, b])] == 0 for s in range(tb.S))
        assert not np.isnan(x[nf[[0, 1, 3]]]).any() and np.isnan(x[nf[2]]).sum() == tb.S
        assert (x[nf[1]] == np.inf).sum() == tb.S and (x[nf[1]] == -np.inf).sum() == tb.S
    elif group == "sub":
        sb = tb.rows_of("subnormal")
        assert sb.size >= 2 and (np.abs(x[sb]) < tiny).all() and (x[sb] != 0).all() and (x[sb] < 0).any() and (x[sb] > 0).any()
        assert (np.abs(exp.ref[sb]) < 64).all() and np.median(np.abs(exp.ref[sb])) > 2.0 ** -8, "the subnormal dots are O(1)"
    else:
        big = float(np.finfo(dc.DTYPES[dtype_name]).max)
        xt = tb.rows_of("extreme")
        assert xt.size >= 2 and (np.abs(x[xt]) > big / 2).all() and (x[xt] < 0).any() and (x[xt] > 0).any() and np.isfinite(exp.mag).all()


@pytest.mark.parametrize("group,dtype_name,D", CASES)
def test_honest_orders_stay_inside_the_bound_and_nothing_is_left_out(expected, group, dtype_name, D):
    tb, exp = expected(group, dtype_name, D)
    n_vec = tb.n * tb.S * tb.E
    n_bad = len(tb.nonfinite_rows) * tb.S                       # one non-finite split per stream of a non-finite row
    assert int(np.isfinite(exp.ref).sum()) == n_vec - n_bad and int(np.isfinite(exp.avg).sum()) == (tb.n - len(tb.nonfinite_rows)) * tb.S
    for name, dot in (("np.dot", dot_numpy), ("sequential", dot_sequential), ("64 lanes + butterfly", dot_lanes)):
        sims = dot(tb)
        avg, n_e = host_results(tb, sims)
        worst, n_fin, n_cls = dc.check_against(exp, tb.family, avg, n_e, sims)
        # every finite (row, vector) pair and every finite mean went through the bound; the rest -- rows the table marks -- through the class check
        assert n_fin == n_vec - n_bad + (tb.n - len(tb.nonfinite_rows)) * tb.S and n_cls == n_bad + len(tb.nonfinite_rows) * tb.S, name
        assert set(worst) == set(dc.GROUP_FAMILIES[group]) and max(worst.values()) <= 1.0
        print("%s %s D=%d %s: %s" % (group, dtype_name, D, name, dc.ratio_line(worst)))
    # under the mask: the non-finite splits are absent, those means finite and inside the bound; a stream without a split is NaN
    m_exp = expected(group, dtype_name, D, masked=True)[1]
    mask = tb.mask()
    assert (mask[tb.nonfinite_rows, :, tb.bad_split] == 0).all() and (mask.sum(axis=2) == 0).sum() >= 2
    assert np.isfinite(m_exp.avg[tb.nonfinite_rows]).all() and (np.isnan(m_exp.avg) == (m_exp.n_e == 0)).all()
    sims = dot_lanes(tb)
    avg, n_e = host_results(tb, sims, mask)
    dc.check_against(m_exp, tb.family, avg, n_e, sims)


# ------------------------------------------------------------------------------------------------------------- wrong dots are told apart
# wrong dot -> (group, type) it is shown on and the family whose rows reject it
REJECTED_BY = {"float32 accumulation": ("plain", "f32", "cancel"),
               "features read as their absolute value": ("plain", "f64", "signs"),
               "float16 subnormals flushed": ("sub", "f16", "subnormal"),
               "float32 subnormals flushed": ("sub", "f32", "subnormal"),
               "mask as a factor": ("plain", "f16", "nonfinite"),
               "NaN row copied into the next row of its tile": ("plain", "f32", "signs"),
               "last 4 elements dropped": ("plain", "f64", "zeros")}


@pytest.mark.parametrize("wrong", list(REJECTED_BY))
@pytest.mark.parametrize("D", DS)
def test_wrong_dots_are_rejected(expected, wrong, D):
    group, dtype_name, family = REJECTED_BY[wrong]
    masked = wrong == "mask as a factor"
    tb, exp = expected(group, dtype_name, D, masked=masked)
    present = tb.mask() if masked else None
    right = dot_sequential(tb)
    assert rejected_families(tb, exp, right, present)[0] == set(), "the honest dot passes"
    skip = True
    if wrong == "float32 accumulation":
        sims = dot_sequential(tb, dtype=np.float32)
    elif wrong == "features read as their absolute value":
        with np.errstate(invalid="ignore"):
            sims = dot_sequential(tb, np.abs(tb.x.astype(np.float64)) * tb.t[None])
    elif wrong.endswith("subnormals flushed"):
        x = tb.x.astype(np.float64)
        x[np.abs(x) < float(np.finfo(tb.dtype).tiny)] = 0.0
        sims = dot_sequential(tb, x * tb.t[None])
    elif masked:
        sims, skip = right, False
    elif wrong.startswith("NaN row"):
        sims = right.copy()
        src = tb.nonfinite_rows[2]                               # the row with a NaN
        assert tb.variant[src] == "nan" and (src + 1) % 16 != 0 and tb.family[src + 1] == "signs"
        sims[src + 1] = sims[src]
    else:
        p = products(tb)
        p[..., -4:] = 0.0                                        # never added (at D = 4: nothing is)
        sims = dot_sequential(tb, p)
    got, bad = rejected_families(tb, exp, sims, present, skip)
    assert family in got, (wrong, got)
    if wrong.startswith("NaN row"):
        assert np.flatnonzero(bad).tolist() == [int(tb.nonfinite_rows[2]) + 1]
    if wrong == "last 4 elements dropped":
        assert {tb.variant[r] for r in np.flatnonzero(bad) if tb.family[r] == "zeros"} >= {str(D - 4), str(D - 1)}
    if wrong.endswith("subnormals flushed"):
        assert bad[tb.rows_of("subnormal")].all() and not bad[tb.rows_of("signs")].any()
    if masked:
        assert bad[tb.nonfinite_rows].all() and got == {"nonfinite"}


def test_query_variants_of_a_batched_pass_change_the_class_not_the_exactness():
    tb = dc.table("plain", "f32", *SHAPE, 256)
    nf = tb.nonfinite_rows
    want = {0: np.inf, 1: -np.inf, 3: -np.inf}
    for q in range(4):
        t = dc.query_variant(tb, q)
        m, _ = np.frexp(t)
        assert (m * 2.0 ** 29 == np.round(m * 2.0 ** 29)).all()
        ref, _mag = dc.exact_dots(tb.x[nf], t)
        got = ref[0, :, tb.bad_split]
        assert np.isnan(got).all() if q == 2 else (got == want[q]).all()
        assert np.isnan(ref[1:, :, tb.bad_split]).all()
