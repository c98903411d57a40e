"""CPU: the forced schedules and the error trace of oracle/tvl1_oracle.py, the input builders of tests/_flow_inputs.py and the
comparison helpers the GPU module (tests/test_flow_edges_gpu.py) judges the kernels with.  The helpers are controls first: each of
them is shown an injected error of the size it exists to catch -- one cell off by 2e-4 px, a schedule one iteration too long, one
iteration too short in one warp of one pair, two pairs of a batch swapped -- and has to fail on it.  The degenerate match sets of
oracle/warp_oracle.ransac_homography (nothing to draw from: identity, 0 inliers, winner -1) are pinned here too."""
import numpy as np
import pytest

import _flow_inputs as fi
import tvl1_oracle as tv
import warp_oracle as wo

H, W = 96, 128
KW = dict(nscales=3, warps=3)


@pytest.fixture(scope="module")
def runs():
    """Three pairs (hard, smooth, hard) under the stopping rule, with their traces: what plays the device in the controls below."""
    pairs = [fi.hard_pair(H, W, seed=1), fi.shifted_pair(H, W, 2.5, -1.0, seed=2), fi.hard_pair(H, W, seed=3)]
    return pairs, [tv.tvl1_flow(f0, f1, trace=True, **KW) for f0, f1 in pairs]


def test_forced_schedule_with_the_oracles_own_counts_is_the_unforced_run(runs):
    pairs, free = runs
    for (f0, f1), (u1, u2, counts, errors) in zip(pairs, free):
        v1, v2, c2, e2 = tv.tvl1_flow(f0, f1, schedule=counts, trace=True, **KW)
        assert fi.same_bits(u1, v1) and fi.same_bits(u2, v2) and c2 == counts and e2 == errors
        w1, w2, c3 = tv.tvl1_flow(f0, f1, **KW)                          # the defaults are what they were: three values, the same bits
        assert fi.same_bits(u1, w1) and fi.same_bits(u2, w2) and c3 == counts
    # a forced schedule overrides the rule in both directions, and epsilon / iterations then decide nothing
    f0, f1 = pairs[1]
    a = tv.tvl1_flow(f0, f1, schedule=[[2, 7, 1]] * 3, epsilon=0.0, iterations=1, **KW)
    b = tv.tvl1_flow(f0, f1, schedule=[[2, 7, 1]] * 3, epsilon=5.0, iterations=300, **KW)
    assert a[2] == [[2, 7, 1]] * 3 and fi.same_bits(a[0], b[0]) and fi.same_bits(a[1], b[1])
    with pytest.raises(ValueError):
        tv.tvl1_flow(f0, f1, schedule=[[2, 7, 1]] * 2, **KW)
    # one level alone
    z = np.zeros((H, W), np.float32)
    u1, u2, ran, errs = tv.tvl1_level(f0, f1, z, z, warps=2, schedule=[3, 5], trace=True)
    assert ran == [3, 5] and [len(e) for e in errs] == [3, 5] and len(tv.tvl1_level(f0, f1, z, z, warps=2, schedule=[3, 5])) == 3


def test_trace_obeys_the_stopping_rule(runs):
    eps2 = float(np.float32(tv.EPSILON)) ** 2
    total = 0
    for _, (_, _, counts, errors) in zip(*runs):
        assert fi.audit_decisions(counts, errors, tv.EPSILON, tv.ITERATIONS, 0.0)[1] == 0        # nothing exempted with d = 0
        for cl, el in zip(counts, errors):
            for k, errs in zip(cl, el):
                assert len(errs) == k and all(e > eps2 for e in errs[:-1]) and (errs[-1] <= eps2 or k == tv.ITERATIONS)
                total += k
    assert total > 300
    # a low cap: the last iteration is the cap's, whatever its error
    f0, f1 = runs[0][0]
    _, _, counts, errors = tv.tvl1_flow(f0, f1, iterations=6, trace=True, **KW)
    assert max(max(c) for c in counts) == 6 and any(e[-1] > eps2 for lvl in errors for e in lvl if len(e) == 6)
    assert fi.audit_decisions(counts, errors, tv.EPSILON, 6, 0.0) == (sum(sum(c) for c in counts), 0)


@pytest.mark.parametrize("shape", [(16, 16), (17, 19), (16, 200), (200, 16), (96, 128)])
def test_every_builder_gives_finite_fields(shape):
    h, w = shape
    pairs = {name: make(h, w, seed=4) for name, make in fi.BUILDERS.items()}
    pairs["hard"] = fi.hard_pair(h, w, seed=4)
    pairs["smooth"] = fi.shifted_pair(h, w, 1.5, -0.5, seed=4)
    for name, (f0, f1) in pairs.items():
        assert f0.shape == f1.shape == (h, w) and f0.dtype == f1.dtype == np.uint8, name
        assert fi.same_bits(fi.BUILDERS[name](h, w, seed=4)[1], f1) if name in fi.BUILDERS else True       # seeded
        u1, u2, counts = tv.tvl1_flow(f0, f1, nscales=2, warps=2, iterations=12)
        assert np.isfinite(u1).all() and np.isfinite(u2).all(), name
        assert np.abs(u1).max() < 4 * max(h, w) and np.abs(u2).max() < 4 * max(h, w), name
    assert (pairs["identical"][0] == pairs["identical"][1]).all() and (pairs["hard"][0] != pairs["hard"][1]).any()
    sat = np.concatenate(pairs["saturated"])
    assert (sat == 0).any() and (sat == 255).any()


def test_hard_inputs_reach_every_case_of_the_thresholding_step():
    """Cells per case (below, above, between with a gradient, between WITHOUT one -- the 0 / 0 the packed form computes and selects
    away) over a whole run: the smooth texture of the older tests never takes the fourth, the hard inputs take all four."""
    hard = [fi.case_counts(*fi.hard_pair(96, 128, seed=s), nscales=3, warps=2, iterations=13, epsilon=0.0) for s in (1, 2, 3)]
    assert all((c > 0).all() for c in hard), hard
    smooth = fi.case_counts(*fi.shifted_pair(96, 128, 2.5, -1.0, seed=2), nscales=3, warps=2, iterations=13, epsilon=0.0)
    assert smooth[3] == 0 and (smooth[:3] > 0).all()
    flat = fi.case_counts(*fi.square_on_black(64, 80, seed=1), nscales=1, warps=1, iterations=4, epsilon=0.0)
    assert flat[3] > flat[:3].sum()                              # almost every cell of a black frame has neither gradient nor residual


# ---- the controls: every helper fails on the error it is there to catch ---------------------------------------------------------

def test_control_one_cell_off_by_2e_4_px(runs):
    _, free = runs
    u1, u2 = free[0][0], free[0][1]
    assert fi.assert_fields_match(u1.copy(), u2.copy(), u1, u2) == 0.0
    for plane in (0, 1):
        bad = [u1.copy(), u2.copy()]
        bad[plane][37, 90] += np.float32(2e-4)
        with pytest.raises(AssertionError):
            fi.assert_fields_match(bad[0], bad[1], u1, u2)
        assert not fi.same_bits(bad[plane], (u1, u2)[plane])
    bad = u1.copy()
    bad[0, 0] = np.nan
    with pytest.raises(AssertionError):
        fi.assert_fields_match(bad, u2, u1, u2)
    assert not fi.same_bits(np.float32([0.0]), np.float32([-0.0])) and fi.same_bits(u1, u1.copy())


def _bump(counts, lvl, wp, by):
    out = [list(c) for c in counts]
    out[lvl][wp] += by
    return out


def test_control_a_schedule_with_one_iteration_more(runs):
    """A device that ran one iteration past the stop (a replay of j + 2): its fields are those of the longer schedule.  Against the
    oracle forced to the counts the rule gives, the field bound fails; against the oracle forced to the device's own (longer) counts the
    fields agree and the AUDIT fails: the iteration before the last was already small enough."""
    pairs, free = runs
    for (f0, f1), (u1, u2, counts, _) in zip(pairs, free):
        for lvl, wp in ((0, 0), (2, 2)):
            longer = _bump(counts, lvl, wp, +1)
            d1, d2, _, trace = tv.tvl1_flow(f0, f1, schedule=longer, trace=True, **KW)            # "the device"
            with pytest.raises(AssertionError):
                fi.assert_fields_match(d1, d2, u1, u2)
            with pytest.raises(AssertionError):
                fi.audit_decisions(longer, trace, tv.EPSILON, tv.ITERATIONS, d=1e-6)


def test_control_one_iteration_fewer_in_one_warp_of_one_pair(runs):
    pairs, free = runs
    (f0, f1), (u1, u2, counts, _) = pairs[2], free[2]
    for lvl, wp in ((1, 1), (2, 0)):
        assert counts[lvl][wp] > 1
        shorter = _bump(counts, lvl, wp, -1)
        d1, d2, _, trace = tv.tvl1_flow(f0, f1, schedule=shorter, trace=True, **KW)
        with pytest.raises(AssertionError):
            fi.assert_fields_match(d1, d2, u1, u2)
        with pytest.raises(AssertionError):
            fi.audit_decisions(shorter, trace, tv.EPSILON, tv.ITERATIONS, d=1e-6)
        # the other pairs of the batch stay right
        assert fi.audit_decisions(free[0][2], free[0][3], tv.EPSILON, tv.ITERATIONS, d=1e-6)[1] == 0


def test_control_two_pairs_swapped(runs):
    _, free = runs
    got = [free[2], free[1], free[0]]                           # a batch whose pairs 0 and 2 came back in each other's place
    with pytest.raises(AssertionError):
        fi.assert_fields_match(got[0][0], got[0][1], free[0][0], free[0][1])
    with pytest.raises(AssertionError):
        fi.assert_fields_match(got[2][0], got[2][1], free[2][0], free[2][1])
    fi.assert_fields_match(got[1][0], got[1][1], free[1][0], free[1][1])
    assert not fi.same_bits(got[0][0], free[0][0])


def test_grazing_band_is_narrow_and_counted():
    """The exemption of audit_decisions: only inside |error / eps^2 - 1| < 4 d / epsilon, and every use of it is counted."""
    eps2 = float(np.float32(0.01)) ** 2
    trace = [[[4.0 * eps2, 0.9995 * eps2, 0.5 * eps2]]]          # the second iteration should have stopped the loop: 5e-4 below
    with pytest.raises(AssertionError):
        fi.audit_decisions([[3]], trace, 0.01, 300, d=1e-6)      # band 4e-4
    assert fi.audit_decisions([[3]], trace, 0.01, 300, d=2e-6) == (3, 1)        # band 8e-4: exempt, and counted
    assert fi.audit_decisions([[3]], [[[4.0 * eps2, 1.0005 * eps2, 0.5 * eps2]]], 0.01, 300, d=0.0) == (3, 0)      # going on was right
    with pytest.raises(AssertionError):
        fi.audit_decisions([[3]], [[[4.0 * eps2, 0.9 * eps2, 0.5 * eps2]]], 0.01, 300, d=1e-4)      # 10 % inside: never grazing
    assert fi.audit_decisions([[3]], [[[4.0 * eps2, 0.99999 * eps2, 0.5 * eps2]]], 0.01, 300, d=1e-6) == (3, 1)
    assert fi.audit_decisions([[3]], [[[4.0 * eps2, 2.0 * eps2, 3.0 * eps2]]], 0.01, 3, d=0.0) == (3, 0)       # the cap stops it
    with pytest.raises(AssertionError):
        fi.audit_decisions([[3]], [[[4.0 * eps2, 2.0 * eps2, 3.0 * eps2]]], 0.01, 300, d=0.0)


# ---- degenerate match sets: what the oracle defines, so that the kernel can be held to it ----------------------------------------

def test_ransac_oracle_on_degenerate_sets_is_identity_zero_minus_one():
    rng = np.random.default_rng(0)
    few = rng.uniform(0, 100, (3, 2)).astype(np.float32)
    same = np.tile(np.float32([[31.5, 40.25]]), (40, 1))
    t = np.arange(40, dtype=np.float32)
    line = np.stack([2 * t, 3 * t + 7], 1).astype(np.float32)         # whole numbers: exactly collinear in fp32 and fp64
    empty = np.zeros((0, 2), np.float32)
    for src, dst in ((few, few + 1), (same, same + 2), (line, line + np.float32([1.0, -2.0])), (empty, empty)):
        for refit in (False, True):
            G, cnt, winner, mask = wo.ransac_homography(src, dst, 1.0, 64, seed=3, pair=1, refit=refit)
            assert (G == np.eye(3)).all() and cnt == 0 and winner == -1 and mask.shape == (len(src),) and mask.sum() == 0
    # exactly four matches in general position: one hypothesis shape, all four are inliers, the refit is the 4-point solution
    H = np.array([[1.02, 0.01, 3.0], [-0.02, 0.99, -2.0], [1e-5, 2e-5, 1.0]])
    src = np.float32([[10, 12], [200, 20], [190, 170], [15, 160]])
    p = np.c_[src, np.ones(4)] @ H.T
    dst = (p[:, :2] / p[:, 2:]).astype(np.float32)
    G, cnt, winner, mask = wo.ransac_homography(src, dst, 1.0, 64, seed=3, pair=0)
    assert cnt == 4 and winner >= 0 and mask.tolist() == [1, 1, 1, 1] and np.abs(G - H).max() < 1e-3
