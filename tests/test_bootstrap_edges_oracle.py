"""CPU: the references of the bootstrap edge tests check each other, and the committed case table (tests/_bootstrap_cases.py) keeps
what it promises -- so that no test of tests/test_bootstrap_edges_gpu.py can pass vacuously:

  * the exact rational target through the Gram form equals the reference's explicit formulas evaluated exactly (small D), for both
    closed forms: the two are one rational function;
  * the kernel-order restatement, the Woodbury route and the explicit-inverse oracle each agree with the exact target on every
    exact case, and all three with each other on the 256-row and wide cases: no case's spread exceeds 1e-12 (measured: at most
    3.0e-14, see the GPU module's table);
  * every "swaps" case really swaps rows in the solve it is named for (counted in the kernel's own elimination order);
  * the kernel's pivot rule, restated, refuses every linearly dependent input the GPU module expects a refusal for.

No GPU, no product code: numpy, stdlib fractions and oracle/bootstrap_oracle.py.  The whole module takes a few seconds; the exact
references take 0.00 - 0.3 s per case (1.3 s for the twelve exact cases of one storage type)."""
import numpy as np
import pytest

import _bootstrap_cases as bc
import bootstrap_oracle as bo

DTYPES = ("float64", "float32")
SPREAD_MAX = 1e-12


def _small(m, n, D, seed, dtype="float64"):
    rng = np.random.default_rng(seed)
    R = (np.abs(rng.standard_normal((m + n, D))) * 10.0 ** rng.uniform(-1.5, 1.5, (m + n, 1))).astype(dtype).astype(np.float64)
    return R[:m], (R[m:] if n else None)


@pytest.mark.parametrize("m,n,D,mu", [(4, 3, 12, 0.3), (4, 3, 12, 40.0), (2, 5, 9, 1.5), (4, 0, 12, 0.0), (1, 0, 5, 0.0), (3, 2, 8, 0.0)])
@pytest.mark.parametrize("dtype", ["float64", "float32", "float16"])
def test_exact_gram_form_equals_exact_explicit_form(m, n, D, mu, dtype):
    X, Y = _small(m, n, D, 100 * m + n, dtype)
    gram = bo.exact_target(X, Y, mu)
    explicit = bo.exact_target_explicit(X, Y, mu)
    assert gram.tobytes() == explicit.tobytes()                 # one rational function, rounded once: identical doubles
    if mu == 0.0 and n:
        assert gram.tobytes() == bo.exact_target(X, None, 0.0).tobytes()


def test_exact_target_is_exact_on_a_problem_with_a_known_answer():
    # orthogonal rows with power-of-two norms: w = sum_i x_i / |x_i|^2, every step exact
    X = np.zeros((3, 8))
    X[0, 0], X[1, 3], X[2, 5] = 2.0, 0.5, 8.0
    want = np.zeros(8)
    want[0], want[3], want[5] = 0.5, 2.0, 0.125
    assert (bo.exact_target(X, None, 0.0) == want).all()
    w, s1, s2 = bo.kernel_order_target(X, None, 0.0)
    assert (w == want).all() and (s1, s2) == (0, 0)
    with pytest.raises(ZeroDivisionError):
        bo.exact_target(np.stack([X[0], X[0]]), None, 0.0)
    with pytest.raises(ZeroDivisionError):
        bo.exact_target(X, np.zeros((2, 8)), 0.3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", bc.EXACT, ids=bc.case_id)
def test_fp64_routes_agree_with_the_exact_target(case, dtype):
    r = bc.references(case, dtype)
    for name in ("kernel", "woodbury", "explicit"):
        d = bc.rel(getattr(r, name), r.exact)
        assert d <= SPREAD_MAX, (name, d)
    assert 0.0 < r.spread <= SPREAD_MAX
    assert r.w_ref is r.exact


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", bc.LARGE, ids=bc.case_id)
def test_fp64_routes_agree_on_the_large_cases(case, dtype):
    r = bc.references(case, dtype)
    assert 0.0 < r.spread <= SPREAD_MAX
    assert r.exact is None and r.w_ref is r.woodbury


@pytest.mark.parametrize("dtype", DTYPES)
def test_swap_cases_swap_in_the_solve_they_are_named_for(dtype):
    for case in bc.SWAPS_FIRST:
        assert bc.references(case, dtype).swaps_first >= 1, case
    for case in bc.SWAPS_SECOND:
        assert bc.references(case, dtype).swaps_second >= 1, case
    # ... and the full-size cases exercise the swap path at scale (the right-hand-side columns sit past column 255 there)
    assert bc.references(bc.FULL[0], dtype).swaps_second >= 50
    assert bc.references(bc.FULL[1], dtype).swaps_second >= 10


def test_rows_of_similar_norm_never_swap():
    """Spread 0 -> the diagonal stays the column maximum in both solves: the swap path needs the spread of the table's cases (or
    the strong common component of real feature rows: the recorded fixtures swap twice in the second solve, never in the first)."""
    for seed in range(5):
        X, Y = bc.rows(bc.Case(12, 8, 260 + 4 * seed, 0, 0.3))
        _, s1, s2 = bo.kernel_order_target(X, Y, 0.3)
        assert (s1, s2) == (0, 0)


@pytest.mark.parametrize("S,E", [(1, 1), (2, 3)])
@pytest.mark.parametrize("D", [64, 260, 1024])
@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
def test_resident_cases_hold_the_same_conditions(S, E, D, dtype):
    x = bc.resident_block(S, E, D, dtype)
    assert x.dtype == np.dtype(dtype) and x.shape == (bc.RES_N, S, E, D)
    assert 0 in bc.RES_VALID and bc.RES_N - 1 in bc.RES_VALID
    for row in bc.resident_references(S, E, D, dtype):
        for r in row:
            assert 0.0 < r.spread <= SPREAD_MAX


def test_scaling_by_a_power_of_two_is_exact_in_kernel_order():
    """What the GPU module asserts of the device holds for the algorithm: rows * 2^k -> w * 2^-k, swaps unchanged."""
    for case in (bc.SWAPS_SECOND[1], bc.SWAPS_FIRST[0]):
        X, Y = bc.rows(case)
        w, s1, s2 = bo.kernel_order_target(X, Y, case.mu)
        for k in (20, -20):
            wk, k1, k2 = bo.kernel_order_target(np.ldexp(X, k), np.ldexp(Y, k), case.mu)
            assert (k1, k2) == (s1, s2)
            assert np.ldexp(wk, k).tobytes() == w.tobytes()


def _dependent(kind, dtype, seed):
    X, Y = _small(6, 4, 68, seed, dtype)
    rng = np.random.default_rng(seed)
    i, pos = int(rng.integers(6)), int(rng.integers(7))
    extra = {"duplicate": X[i], "double": 2.0 * X[i], "zero": 0.0 * X[i], "sum": X[0] + X[1]}[kind]
    return np.insert(X, pos, extra, axis=0), Y


@pytest.mark.parametrize("kind", ["duplicate", "double", "zero"])
def test_pivot_rule_refuses_dependent_rows(kind):
    """A repeated row (or a power-of-two multiple) leaves a column of rounding residue, not of zeros: identical columns stay
    identical bit for bit until one is eliminated, and the other is then left with a - fl(a * fl(v * fl(1 / v))), 0 or an ulp of a.
    The test ``pivot > 0`` alone let such systems through (next test); the floor of csrc/vq_boot.hip (dim * 16 eps * the column's
    largest entry) refuses all of them, with and without non-matches, in every storage type.  (A general dependence, x_a = x_b +
    x_c, is refused as well unless the other rows are themselves nearly dependent -- its residue carries their condition number:
    67 of 72 such systems here.  Rank decisions at cond ~ 1/eps are beyond any pivot test, LAPACK's included.)"""
    for dtype in ("float64", "float32", "float16"):
        for seed in range(12):
            X, Y = _dependent(kind, dtype, seed)
            for Yy, mu in ((None, 0.0), (Y, 0.3)):
                with pytest.raises(bo.SingularSystem):
                    bo.kernel_order_target(X, Yy, mu)


def test_without_the_floor_dependent_rows_slip_through(monkeypatch):
    """The finding itself, kept reproducible: with the floor at 0 (the kernel as it was) some of the same systems are 'solved'."""
    monkeypatch.setattr(bo, "PIVOT_TOL_PER_ROW", 0.0)
    passed = 0
    for kind in ("duplicate", "double"):
        for seed in range(12):
            X, Y = _dependent(kind, "float32", seed)
            try:
                bo.kernel_order_target(X, None, 0.0)
                passed += 1
            except bo.SingularSystem:
                pass
    assert passed >= 1
    # the inputs the GPU module sends were picked among those: a kernel without the floor returns a target for each of them
    for kind in ("duplicate", "double"):
        X, Y, mu = bc.dependent_host(kind)
        bo.kernel_order_target(X, Y, mu)
    for dtype, (valid, mu) in bc.RES_TWICE.items():
        x = bc.resident_block(1, 1, 260, dtype).astype(np.float64)[:, 0, 0]
        bo.kernel_order_target(x[valid], x[list(bc.RES_INVALID)] if mu else None, mu)


def test_the_dependent_inputs_of_the_gpu_module_are_refused_in_kernel_order():
    for kind in ("duplicate", "double"):
        X, Y, mu = bc.dependent_host(kind)
        with pytest.raises(bo.SingularSystem):
            bo.kernel_order_target(X, Y, mu)
    for dtype, (valid, mu) in bc.RES_TWICE.items():
        x = bc.resident_block(1, 1, 260, dtype).astype(np.float64)[:, 0, 0]
        with pytest.raises(bo.SingularSystem):
            bo.kernel_order_target(x[valid], x[list(bc.RES_INVALID)] if mu else None, mu)


def test_pivot_floor_is_far_below_every_accepted_pivot():
    """The floor must never refuse a system the suite solves: on every case of the table the smallest accepted pivot, relative to
    its column's largest original entry, stays at least 1e6 times above the floor (measured: 5.3e9 times on the table, 3.2e11 /
    3.6e9 on the recorded real / synthetic fixtures of tests/test_bootstrap_gpu.py)."""
    worst = np.inf
    for case in bc.ALL:
        X, Y = bc.rows(case)
        worst = min(worst, _pivot_headroom(X, Y, case.mu))
    assert worst >= 1e6, worst


def _pivot_headroom(X, Y, mu):
    """min over both solves and all steps of pivot / floor, from a traced copy of the oracle's elimination."""
    seen = []
    orig = bo._kernel_gauss_jordan

    def traced(aug, dim):
        a = aug.copy()
        floor = (bo.PIVOT_TOL_PER_ROW * dim) * np.abs(a[:, :dim]).max(axis=0)
        for k in range(dim):
            p = k + int(np.argmax(np.abs(a[k:, k])))
            seen.append(abs(a[p, k]) / floor[k])
            a[[k, p]] = a[[p, k]]
            a[k] *= 1.0 / a[k, k]
            others = np.arange(dim) != k
            a[others, k + 1:] -= np.outer(a[others, k], a[k, k + 1:])
            a[others, k] = 0.0
        return orig(aug, dim)

    bo._kernel_gauss_jordan = traced
    try:
        bo.kernel_order_target(X, Y, mu)
    finally:
        bo._kernel_gauss_jordan = orig
    return min(seen)


def test_refusals_of_non_finite_and_degenerate_input_in_kernel_order():
    X, Y = _small(6, 4, 64, 3)
    with pytest.raises(bo.SingularSystem):                      # mu / tr(0) = inf -> NaN pivots
        bo.kernel_order_target(X, 0.0 * Y, 0.3)
    Xi = X.copy()
    Xi[2, 5] = np.inf
    with pytest.raises(bo.SingularSystem):
        bo.kernel_order_target(Xi, Y, 0.3)
    with pytest.raises(bo.SingularSystem):
        bo.kernel_order_target(Xi, None, 0.0)
    w, _, _ = bo.kernel_order_target(X, 0.0 * Y, 0.0)         # mu = 0: the non-matches do not enter
    assert w.tobytes() == bo.kernel_order_target(X, None, 0.0)[0].tobytes()


def test_scaled_query_reference():
    r = np.array([3.0, 4.0, 0.0, 0.0])
    assert (bc.scaled_query_exact(r) == r / 25.0).all()
