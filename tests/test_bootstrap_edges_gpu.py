"""GPU: the bootstrap kernel (csrc/vq_boot.hip) and scale_query_kernel (csrc/vq_db.hip) at the edges, to the accuracy of their own
arithmetic.  tests/test_bootstrap_gpu.py holds them to the reference's recorded fixtures within 1e-8 (the conditioning of those
fixtures through explicit 1024 x 1024 inverses); here the bound is what fp64 roundings of ONE formula can differ by.

Accuracy rule.  |w_gpu - w_ref|_max <= 8 * spread * max|w_ref|, where spread is computed from CPU references alone
(tests/_bootstrap_cases.py):
  cases up to 20 rows   w_ref = the exact rational target, rounded once; spread = the largest relative distance from it of the
                        kernel-order restatement, the Woodbury route (BLAS + LAPACK) and the explicit-inverse oracle
  256-row / wide cases  w_ref = the Woodbury route; spread = the largest pairwise relative distance of those three
All are O(cond * eps) roundings of the same rational function; the device differs from the kernel-order restatement only where the
compiler may differ from numpy, i.e. nowhere by construction (the library is built without contraction).  8 is the margin for that.
tests/test_bootstrap_edges_oracle.py asserts on the CPU that every spread is <= 1e-12 and that the "swaps" cases swap.

Measured on the CPU (fp64 values; fp32 values give the same magnitudes), spread and row swaps (first solve, second solve):
  m3-n2-D4-s1.5-mu0.3      9.6e-15  0   2        m1-n0-D64-s1.5          1.4e-16  0   0
  m6-n4-D64-s1.5-mu0.3     1.1e-15  0   3        m1-n1-D64-s1.5-mu0.3    6.6e-16  0   0
  m6-n4-D68-s1.5-mu0.3     1.9e-15  0   3        m1-n19-D68-s1-mu0.3     5.6e-16  0   0
  m12-n8-D100-s1.5-mu0.3   2.1e-15  0  10        m256-n0-D1024-s1        2.4e-14  0 161
  m12-n8-D260-s1.5-mu0.3   3.3e-15  0   6        m128-n128-D1024-s1-mu0.3 1.7e-14 0  53
  m9-n0-D260-s2            2.7e-15  0   5        m1-n255-D1024-s1-mu0.3  1.7e-15  0   0
  m12-n8-D260-s2-mu1.5     3.2e-15  0  11        m255-n1-D1024-s0-mu1.5  2.5e-14  0   0
  m6-n10-D64-s1.5-mu40     1.4e-15  2   1        m100-n156-D260-s1-mu0.3 2.1e-14  0  66
  m6-n10-D64-s1.5-mu400    6.5e-15  1   1        m5-n3-D2048-s1-mu0.3    4.5e-15  0   1
Resident cases (7 rows per slot, exact reference): spreads 4e-16 .. 3.4e-15.

Exact properties are asserted bit for bit; refusals are status returns of a kernel that completes (no device fault involved)."""
import math

import numpy as np
import pytest

import _bootstrap_cases as bc

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
NP = {"float16": np.float16, "float32": np.float32, "float64": np.float64}


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


@pytest.fixture(scope="module")
def solve(vqa):
    from video_query_algorithms_amd.bootstrap import bootstrap_targets
    return bootstrap_targets


def _as(X, Y, dtype):
    """The case's values in their storage type (an exact narrowing: they were rounded to it when they were made)."""
    return X.astype(NP[dtype]), (None if Y is None else Y.astype(NP[dtype]))


def _check_accuracy(w, refs, what):
    scale = float(np.abs(refs.w_ref).max())
    err = float(np.abs(w - refs.w_ref).max())
    allowed = bc.MARGIN * refs.spread * scale
    print("%s: |dw|/max|w| %.2e, spread %.2e, %.2f of the allowance" % (what, err / scale, refs.spread, err / allowed))
    assert np.isfinite(w).all()
    assert err <= allowed, (what, err / scale, refs.spread)


# ------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", bc.ALL, ids=bc.case_id)
def test_host_rows_accuracy(solve, case, dtype):
    X, Y = bc.rows(case, dtype)
    w = solve([_as(X, Y, dtype)], case.mu)[0]
    _check_accuracy(w, bc.references(case, dtype), bc.case_id(case) + " " + dtype)


@pytest.mark.parametrize("case", bc.ALL, ids=bc.case_id)
def test_validated_matches_score_one(solve, case):
    """X w = 1 (both closed forms), within 8 * cond(Gxx) * eps; the product is taken in extended precision."""
    X, Y = bc.rows(case)
    w = solve([(X, Y)], case.mu)[0]
    res = float(np.abs((X.astype(np.longdouble) @ w.astype(np.longdouble)) - 1).max())
    cond = float(np.linalg.cond(X @ X.T))
    print("%s: |Xw - 1| %.2e, cond(Gxx) %.2e, %.3f of the allowance" % (bc.case_id(case), res, cond, res / (bc.MARGIN * cond * EPS)))
    assert res <= bc.MARGIN * cond * EPS


# ------------------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", [bc.SWAPS_SECOND[1], bc.TAILS[0], bc.SINGLE[2], bc.FULL[1]], ids=bc.case_id)
def test_mu_zero_ignores_the_non_matches(solve, case, dtype):
    X, Y = _as(*bc.rows(case, dtype), dtype)
    alone = solve([(X, None)], 0.0)[0]
    assert solve([(X, Y)], 0.0)[0].tobytes() == alone.tobytes()
    assert solve([(X, np.zeros_like(Y))], 0.0)[0].tobytes() == alone.tobytes()        # ... whatever they are
    assert solve([(X, None)], case.mu)[0].tobytes() == alone.tobytes()                  # and mu without non-matches is not used


@pytest.fixture(scope="module")
def ragged(solve):
    probs = bc.ragged_launch()
    alone = [solve([p], 0.3)[0] for p in probs]
    return probs, alone


def test_problem_inside_a_launch_equals_the_problem_alone(solve, ragged):
    """54 ragged problems, one of 256 rows beside 1-row ones: each has its own scratch region at ws + p * ws_stride, sized by the
    largest; any overlap or a count read from a neighbour's slot changes somebody's bits.  Both orders, so that the 256-row problem
    sits at two positions (and the second launch repeats the first's problems: the same bits again)."""
    probs, alone = ragged
    sizes = [(x.shape[0], 0 if y is None else y.shape[0]) for x, y in probs]
    assert len(probs) == 54 and (128, 128) in sizes and sizes.count((1, 0)) >= 6 and len(set(sizes)) >= 20
    together = solve(probs, 0.3)
    for p in range(len(probs)):
        assert together[p].tobytes() == alone[p].tobytes(), (p, sizes[p])
    back = solve(probs[::-1], 0.3)[::-1]
    assert sizes.index((128, 128)) != len(probs) - 1 - sizes.index((128, 128))
    assert np.ascontiguousarray(back).tobytes() == together.tobytes()
    assert solve(probs, 0.3).tobytes() == together.tobytes()                              # a repeated call reproduces its bits


def test_ragged_launch_is_accurate_too(solve, ragged):
    probs, alone = ragged
    for (X, Y), w in list(zip(probs, alone))[:12]:
        if X.shape[0] + (0 if Y is None else Y.shape[0]) <= 20:
            _check_accuracy(w, bc.references_of(X, Y, 0.3, True), "ragged %d+%d" % (X.shape[0], 0 if Y is None else Y.shape[0]))


@pytest.mark.parametrize("k", [20, -20])
@pytest.mark.parametrize("case", [bc.SWAPS_SECOND[1], bc.SWAPS_FIRST[0], bc.SWAPS_SECOND[0], bc.FULL[4]], ids=bc.case_id)
def test_power_of_two_scaling_is_exact(solve, case, k):
    """rows * 2^k -> w * 2^-k bit for bit: every intermediate scales by a power of two (the Gram matrix by 4^k, s by 4^-k, the
    pivot floor with its column), so pivot choices and roundings are those of the unscaled problem."""
    X, Y = bc.rows(case)
    w = solve([(X, Y)], case.mu)[0]
    wk = solve([(np.ldexp(X, k), None if Y is None else np.ldexp(Y, k))], case.mu)[0]
    assert np.ldexp(wk, k).tobytes() == w.tobytes()


# ---------------------------------------------------------------------------------------------------------- resident path
def _db(vqa, S, E, D, dtype, tiled=False):
    x = bc.resident_block(S, E, D, dtype)
    db = vqa.FeatureDB.from_arrays(x, dtype=NP[dtype])
    if tiled:
        db.set_layout("tiled")
        assert db.layout == "tiled"
    return x, db


def _host_route(solve, x, valid, invalid, mu):
    """The same values through bootstrap_targets (halves widened to fp32: exact), problems in the resident order p = s * E + e."""
    xs = x.astype(np.float32) if x.dtype == np.float16 else x
    S, E = x.shape[1:3]
    probs = [(xs[list(valid), s, e], xs[list(invalid), s, e] if len(invalid) else None) for s in range(S) for e in range(E)]
    return solve(probs, mu).reshape(S, E, -1)


@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
@pytest.mark.parametrize("D", [64, 260, 1024])
@pytest.mark.parametrize("S,E", [(1, 1), (2, 3)])
def test_resident_rows(vqa, solve, S, E, D, dtype):
    x, db = _db(vqa, S, E, D, dtype)
    try:
        t = db.bootstrap_target(bc.RES_VALID, bc.RES_INVALID, mu=bc.RES_MU, set_query=False)
        refs = bc.resident_references(S, E, D, dtype)
        for s in range(S):
            for e in range(E):
                _check_accuracy(t[s, e], refs[s][e], "resident %s S%d E%d D%d slot (%d,%d)" % (dtype, S, E, D, s, e))
        assert t.tobytes() == _host_route(solve, x, bc.RES_VALID, bc.RES_INVALID, bc.RES_MU).tobytes()
        if D == 260:                                                                     # the first closed form, rows 0 and n - 1 again
            t0 = db.bootstrap_target(bc.RES_VALID, mu=bc.RES_MU, set_query=False)
            refs0 = bc.resident_references(S, E, D, dtype, False)
            for s in range(S):
                for e in range(E):
                    _check_accuracy(t0[s, e], refs0[s][e], "resident valid-only %s slot (%d,%d)" % (dtype, s, e))
            assert t0.tobytes() == _host_route(solve, x, bc.RES_VALID, (), 0.0).tobytes()
    finally:
        db.close()


@pytest.mark.parametrize("S,E", [(1, 1), (2, 3)])
def test_tiled_layout_equals_rows_bit_for_bit(vqa, S, E):
    x, rows_db = _db(vqa, S, E, 1024, "float32")
    _, tiled_db = _db(vqa, S, E, 1024, "float32", tiled=True)
    try:
        for invalid, mu in ((bc.RES_INVALID, bc.RES_MU), ((), 0.0)):
            a = rows_db.bootstrap_target(bc.RES_VALID, invalid, mu=mu, set_query=False)
            b = tiled_db.bootstrap_target(bc.RES_VALID, invalid, mu=mu, set_query=False)
            assert a.tobytes() == b.tobytes()
        for row in (0, bc.RES_N - 1):
            assert rows_db.set_query_from_row(row).tobytes() == tiled_db.set_query_from_row(row).tobytes()
    finally:
        rows_db.close()
        tiled_db.close()


@pytest.mark.parametrize("S,E,D,dtype,tiled", [(2, 3, 1024, "float32", False), (2, 3, 1024, "float32", True), (1, 1, 260, "float64", False),
                                               (2, 3, 64, "float16", False)])
def test_set_query_hands_the_target_to_the_next_scan(vqa, S, E, D, dtype, tiled):
    x, db = _db(vqa, S, E, D, dtype, tiled)
    weights = [1.0, 1.5][:S]
    try:
        t = db.bootstrap_target(bc.RES_VALID, bc.RES_INVALID, mu=bc.RES_MU, set_query=True)
        db.scan(weights)
        avg_a, _ = db.similarities()
        sc_a = db.scores().copy()
        db.set_query_from_row(0, want=False)                 # something else in between
        db.set_query(t)
        db.scan(weights)
        avg_b, _ = db.similarities()
        assert avg_a.tobytes() == avg_b.tobytes() and sc_a.tobytes() == db.scores().tobytes()
        assert np.abs(avg_a[list(bc.RES_VALID)] - 1.0).max() <= 1e-9               # and it IS the target: validated matches at 1
        t2 = db.bootstrap_target(bc.RES_VALID, bc.RES_INVALID, mu=bc.RES_MU, set_query=False)
        assert t2.tobytes() == t.tobytes()
    finally:
        db.close()


# --------------------------------------------------------------------------------------------------------------- refusals
def _refused(vqa, fn, text):
    with pytest.raises(vqa.VqError) as e:
        fn()
    assert e.value.code == -1 and "VQ_E_INVALID" in str(e.value) and text in str(e.value), str(e.value)


def _still_correct(solve):
    case = bc.TAILS[2]
    X, Y = bc.rows(case)
    _check_accuracy(solve([(X, Y)], case.mu)[0], bc.references(case), "after a refusal")


SINGULAR = "singular system (linearly dependent validated clips)"


def test_row_limit(vqa, solve):
    rng = np.random.default_rng(257)
    R = np.abs(rng.standard_normal((257, 64)))
    _refused(vqa, lambda: solve([(R[:200], R[200:])], 0.3), "problem 0: 200 + 57 validated clips (limit 256)")
    _refused(vqa, lambda: solve([(R[:3], None), (R, None)], 0.0), "problem 1: 257 + 0 validated clips (limit 256)")
    _still_correct(solve)


def test_no_validated_match(vqa, solve):
    X, Y = bc.rows(bc.TAILS[2])
    _refused(vqa, lambda: solve([(np.zeros((0, 68)), Y)], 0.3), "problem 0: bootstrapping needs at least one validated match")
    _refused(vqa, lambda: solve([(X, Y), (np.zeros((0, 68)), Y)], 0.3), "problem 1: bootstrapping needs at least one validated match")
    _refused(vqa, lambda: solve([(np.zeros((0, 68)), None)], 0.3), "no rows")
    _still_correct(solve)


@pytest.mark.parametrize("kind", ["duplicate", "double"])
def test_dependent_rows_are_refused(vqa, solve, kind):
    """These inputs leave a non-zero residue where the pivot should vanish (asserted on the CPU): without the pivot floor the
    kernel returns a finite target for them."""
    X, Y, mu = bc.dependent_host(kind)
    _refused(vqa, lambda: solve([(X, Y)], mu), "problem 0: " + SINGULAR)
    _refused(vqa, lambda: solve([(X.astype(np.float32), None)], mu), SINGULAR)
    Xc, Yc = bc.rows(bc.DEPENDENT)
    _refused(vqa, lambda: solve([(Xc, Yc), (X, Yc)], 0.3), "problem 1: " + SINGULAR)         # beside a sound problem, with non-matches
    _refused(vqa, lambda: solve([(np.stack([Xc[0], Xc[0]] if kind == "duplicate" else [Xc[0], 2 * Xc[0]]), None)], 0.0), SINGULAR)
    _still_correct(solve)


def test_zero_rows_and_non_finite_input(vqa, solve):
    X, Y = bc.rows(bc.TAILS[2])
    _refused(vqa, lambda: solve([(X, np.zeros_like(Y))], 0.3), SINGULAR)                  # mu / tr(0): a refusal, not a NaN target
    _refused(vqa, lambda: solve([(X.astype(np.float32), np.zeros_like(Y, dtype=np.float32))], 0.3), SINGULAR)
    Z = X.copy()
    Z[3] = 0.0
    _refused(vqa, lambda: solve([(Z, Y)], 0.3), SINGULAR)
    for bad in (np.inf, -np.inf, np.nan):
        Xi = X.copy()
        Xi[2, 5] = bad
        _refused(vqa, lambda: solve([(Xi, Y)], 0.3), SINGULAR)
        _refused(vqa, lambda: solve([(Xi, None)], 0.0), SINGULAR)
        _refused(vqa, lambda: solve([(Xi.astype(np.float32), None)], 0.0), SINGULAR)
        Yi = Y.copy()
        Yi[1, 67] = bad                                                                   # in the tail of both strided loops
        _refused(vqa, lambda: solve([(X, Yi)], 0.3), SINGULAR)
    _still_correct(solve)


@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
def test_resident_refusals(vqa, dtype):
    x, db = _db(vqa, 1, 1, 260, dtype)
    try:
        valid, mu = bc.RES_TWICE[dtype]
        _refused(vqa, lambda: db.bootstrap_target(valid, bc.RES_INVALID if mu else (), mu=mu), SINGULAR)       # one row twice
        _refused(vqa, lambda: db.bootstrap_target([3, 3], mu=0.0), SINGULAR)
        _refused(vqa, lambda: db.bootstrap_target([0, bc.RES_N], mu=0.0), "valid row %d outside [0,%d)" % (bc.RES_N, bc.RES_N))
        _refused(vqa, lambda: db.bootstrap_target([0], [-1], mu=0.3), "invalid row -1 outside [0,%d)" % bc.RES_N)
        _refused(vqa, lambda: db.bootstrap_target([], [1], mu=0.3), "need >= 1 validated match")
        many = [i % bc.RES_N for i in range(257)]
        _refused(vqa, lambda: db.bootstrap_target(many, mu=0.0), "257 + 0 validated clips (limit 256)")
        t = db.bootstrap_target(bc.RES_VALID, bc.RES_INVALID, mu=bc.RES_MU)                                     # the handle still works
        _check_accuracy(t[0, 0], bc.resident_references(1, 1, 260, dtype)[0][0], "resident after refusals " + dtype)
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------------- set_query_from_row
QN = 17          # a ragged last tile of 16 in the tiled layout


@pytest.mark.parametrize("dtype,D,tiled", [(t, d, False) for t in ("float16", "float32", "float64") for d in (4, 64, 260, 2048)]
                         + [("float32", 1024, True), ("float32", 1024, False)])
def test_set_query_from_row(vqa, dtype, D, tiled):
    """t = r / (r . r) against the exact quotient rounded once.  The bound is derived: a thread sums ceil(D / 256) fused terms, the
    wave tree adds 6 levels and the four wave sums take 3 adds, all terms non-negative -> rr is within (ceil(D / 256) + 9) * 2^-53;
    one more rounding for the division and one for the reference's own."""
    S, E = 2, 3
    rng = np.random.default_rng(900 + D)
    x = (np.abs(rng.standard_normal((QN, S, E, D))) * 10.0 ** rng.uniform(-1, 1, (QN, S, E, 1))).astype(NP[dtype])
    db = vqa.FeatureDB.from_arrays(x, dtype=NP[dtype])
    if tiled:
        db.set_layout("tiled")
    bound = (math.ceil(D / 256) + 11) * 2.0 ** -53
    try:
        for row in (0, QN - 1):
            t = db.set_query_from_row(row)
            worst = 0.0
            for s in range(S):
                for e in range(E):
                    want = bc.scaled_query_exact(x[row, s, e].astype(np.float64))
                    worst = max(worst, float((np.abs(t[s, e] - want)[want != 0] / np.abs(want[want != 0])).max()))
                    assert (np.abs(t[s, e] - want) <= bound * np.abs(want)).all()
            print("set_query_from_row %s D%d row %d%s: %.2f of the bound" % (dtype, D, row, " tiled" if tiled else "", worst / bound))
        _refusal = "row %d outside [0,%d)" % (QN, QN)
        _refused(vqa, lambda: db.set_query_from_row(QN), _refusal)
    finally:
        db.close()
