"""GPU: the step between the two flow passes of the warped flow (csrc/vq_flow.hip: corner_strength_kernel, corner_peaks_kernel,
move_corners_kernel, ransac_homography_kernel, homography_warp_kernel, the guards of vq_flow_warped; csrc/host/vq_corners.cc) on the
inputs of tests/_warp_inputs.py, whose properties tests/test_warp_edges_oracle.py shows on the CPU: frame sizes that are no multiple
of the 256-thread block, peaks next to the border, exact ties, a maximum from the last partial block, strong beside weak frames in
a full handle; match sets without a winner, of 4 and 5 and 8192 matches, hypothesis counts around the thread stride, a batch with an
empty set in its middle and NaN beyond every count; whole-pixel and perspective warps; a batch that takes the identity fallback.

PARITY UNPINNED with respect to the reference (third-party extract_warp_gpu, absent): oracle/warp_oracle.py and oracle/tvl1_oracle.py
are the yardstick.  Bars: corners -- the same list bit for bit; RANSAC -- winner, count and mask equal, matrix to 1e-9 relative (the
bound of tests/test_warp_gpu.py); a whole-pixel warp -- the same bits as the flow of the shifted frame; a perspective warp -- 1e-4 px,
the fixed-count bound of tests/test_flow_gpu.py; the one-call warped flow against its steps -- the tolerances of
test_one_call_warped_flow_equals_the_steps.

Found by the binary-noise frames at 37 x 53 and 300 x 16: corner_strength_kernel took its square root with __fsqrt_rn, which this
toolchain maps to the 1-ulp native instruction; two strengths one ulp apart in the oracle came out equal on the device and the corner
list changed its order.  The kernel now calls sqrtf.

Measured on an MI355X (printed by the tests with -s): perspective warp |d| 0 px for both matrices; the one call against its steps
0 px, 0 grey levels; the module takes 5.2 s, its slowest test 0.6 s.

What a one-line change of the code would break (reasoned, not committed): reflect101 mirroring about the edge instead of the last
pixel, or the tie order of the selection sort reversed -> test_corners_of_every_family_and_parameter_at_small_sizes; the RANSAC
reduction preferring the higher index among equals -> the thread-stride and largest-launch tests; the pair term dropped from the
sample hash -> the batch test in two orders; hinv + p * 9 -> hinv -> the whole-pixel translation test (two matrices per batch);
"<= 50 matches" -> "< 50" -> test_warped_guards_and_identity_fallback (pair (c) has exactly 50 matches and more than 25 inliers).
No input here lands on exactly 25 inliers, so "<= 25" against "< 25" is not pinned; a dead lane of corner_strength_kernel computes
pixel (0, 0) of its own frame, so dropping its `live` guard on the block maximum changes nothing any test could see."""
import ctypes as C

import numpy as np
import pytest

import _warp_inputs as wi
import tvl1_oracle as tv
import warp_oracle as wo
from _flow_inputs import same_bits

pytestmark = pytest.mark.gpu
EYE = np.eye(3)


@pytest.fixture(scope="module")
def flow_mod(gpu):
    from video_query_algorithms_amd.tsn import flow
    return flow


# ---- 1. corners ------------------------------------------------------------------------------------------------------------------

def _assert_corners(corners, counts, frames, cap, q, md, what):
    for i, f in enumerate(frames):
        want = wi.oracle_corners(f, cap, q, md)
        assert counts[i] == len(want), (what, i, cap, q, md, int(counts[i]), len(want))
        assert same_bits(corners[i, :counts[i]], want), (what, i, cap, q, md)
        assert (corners[i, counts[i]:] == 0).all(), (what, i)


@pytest.mark.parametrize("shape", wi.SMALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_corners_of_every_family_and_parameter_at_small_sizes(flow_mod, shape):
    h, w = shape
    fr = wi.small_frames(h, w)
    names, frames = list(fr), np.stack(list(fr.values()))
    m = flow_mod.Tvl1Flow(len(frames), h, w)
    for cap, q, md in wi.CORNER_PARAMS:
        corners, counts = m.good_features(frames, cap, q, md)
        _assert_corners(corners, counts, frames, cap, q, md, shape)
        assert counts[names.index("flat")] == 0
    m.close()


def test_corners_of_a_full_size_frame_reach_the_cap(flow_mod):
    f = wi.full_frame()
    m = flow_mod.Tvl1Flow(1, *wi.FULL_SIZE)
    corners, counts = m.good_features(f[None])
    m.close()
    assert counts[0] == 1000
    _assert_corners(corners, counts, f[None], wo.MAX_CORNERS, wo.QUALITY, wo.MIN_DISTANCE, "full size")


def test_corner_maximum_stays_with_its_frame_and_its_call(flow_mod):
    """A handle filled to max_pairs with [strong, weak, noise, strong]: the weak frame keeps its own threshold (with the strong frame's
    it would lose every corner), the same frame first and last gives one list, and a call with one weak frame after the full call gives
    what a fresh handle gives.  Then the same batch from device memory through the raw entry."""
    import torch
    from video_query_algorithms_amd import _lib
    _lib.require_torch_runtime("this test")
    b = wi.leak_batch()
    n, h, w = b.shape
    m = flow_mod.Tvl1Flow(n, h, w)
    assert m.max_pairs == n
    corners, counts = m.good_features(b)
    _assert_corners(corners, counts, b, wo.MAX_CORNERS, wo.QUALITY, wo.MIN_DISTANCE, "full handle")
    assert counts[1] > 10 and counts[0] == counts[3] and same_bits(corners[0], corners[3])
    after, c_after = m.good_features(b[1:2])                                      # slot 0 held the strong frame a call ago
    fresh_m = flow_mod.Tvl1Flow(n, h, w)
    fresh, c_fresh = fresh_m.good_features(b[1:2])
    fresh_m.close()
    assert c_after[0] == c_fresh[0] == counts[1] and same_bits(after, fresh) and same_bits(after[0], corners[1])
    for cap, q, md in ((1000, 0.5, 2.5), (25, 0.001, 4.5)):
        t = torch.from_numpy(b[::-1].copy()).cuda()                               # [strong, noise, weak, strong] on the device
        out, cnt = np.zeros((n, cap, 2), np.float32), np.zeros(n, np.int32)
        _lib.call("vq_flow_good_features", m._h, t.data_ptr(), 1, n, cap, q, md, out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), None)
        _assert_corners(out, cnt, b[::-1], cap, q, md, "frames on the device")
        assert (t.cpu().numpy() == b[::-1]).all()
    m.close()


# ---- 2. RANSAC -------------------------------------------------------------------------------------------------------------------

def _assert_ransac(r, i, src, dst, hyp, seed, pair, refit, what):
    """Set i of a device result against the oracle called with pair = `pair`; -> the oracle's (winner, count)."""
    G, cnt, winner, mask = wo.ransac_homography(src, dst, wi.THRESHOLD, hyp, seed=seed, pair=pair, refit=refit)
    n = len(src)
    assert (int(r["winner"][i]), int(r["inliers"][i])) == (winner, cnt), (what, refit, int(r["winner"][i]), int(r["inliers"][i]), winner, cnt)
    assert (r["mask"][i, :n] == mask).all() and r["mask"][i, n:].sum() == 0, (what, refit)
    d = np.abs(r["H"][i] - G).max()
    assert d <= 1e-9 * np.abs(G).max(), (what, refit, d)
    if winner < 0:
        assert cnt == 0 and (r["H"][i] == EYE).all() and r["mask"][i].sum() == 0, what
    return winner, cnt


def _run_sets(m, sets, mp, hyp, seed, what):
    src, dst, counts = wi.pack(sets, mp)
    out = []
    for refit in (False, True):
        r = m.ransac_homography(src, dst, counts, wi.THRESHOLD, hyp, seed=seed, refit=refit)
        out = [_assert_ransac(r, i, s, d, hyp, seed, i, refit, (what, i)) for i, (s, d) in enumerate(sets)]
    return out


def test_ransac_sets_without_a_winner(flow_mod):
    nw = wi.no_winner_sets()
    m = flow_mod.Tvl1Flow(2, 32, 32)
    for seed in (0, 21):
        got = _run_sets(m, list(nw.values()), 64, 300, seed, "no winner")
        assert got == [(-1, 0)] * len(nw)
    for name, (s, d) in nw.items():                                                # each alone, at the smallest launch that holds it
        assert _run_sets(m, [(s, d)], max(4, len(s)), 7, 5, name) == [(-1, 0)]
    m.close()


def test_ransac_four_and_five_matches(flow_mod):
    small = wi.small_sets()
    m = flow_mod.Tvl1Flow(2, 32, 32)
    assert _run_sets(m, [small["n=4"], small["n=5"]], 5, 64, 21, "small")[1][1] == 5
    assert _run_sets(m, [small["n=4"]], 4, 64, 21, "four alone") == [(0, 4)]
    assert _run_sets(m, [small["n=5"]], 5, 64, 21, "five alone") == [(0, 5)]
    m.close()


def test_ransac_at_the_largest_launch(flow_mod):
    """max_points = 8192: 128 KB of dynamic LDS beside the static arrays, all of it read; then the same arrays with 4000 counted."""
    s, d, _ = wi.full_set()
    m = flow_mod.Tvl1Flow(2, 32, 32)
    assert _run_sets(m, [(s, d)], 8192, 64, 7, "8192 of 8192")[0][1] == 6000
    src, dst = s[None].copy(), d[None].copy()
    for refit in (False, True):
        r = m.ransac_homography(src, dst, np.array([4000], np.int32), wi.THRESHOLD, 64, seed=7, refit=refit)
        _assert_ransac(r, 0, s[:4000], d[:4000], 64, 7, 0, refit, "4000 of 8192")
    m.close()


def test_ransac_hypothesis_counts_around_the_thread_stride(flow_mod):
    s, d = wi.stride_set()
    m = flow_mod.Tvl1Flow(2, 32, 32)
    for hyp in wi.STRIDE_HYPOTHESES:
        got = _run_sets(m, [(s, d)], 320, hyp, wi.STRIDE_SEED, "%d hypotheses" % hyp)
        assert got[0][0] >= 0
    for hyp, (none, first) in wi.FEW_SEEDS.items():                                # idle threads only, and a winner in thread 0
        assert _run_sets(m, [(s, d)], 320, hyp, none, "%d hypotheses, all rejected" % hyp) == [(-1, 0)]
        assert _run_sets(m, [(s, d)], 320, hyp, first, "%d hypotheses, the first wins" % hyp)[0][0] == 0
    assert _run_sets(m, [(s, d)], 320, 2, 1, "2 hypotheses, the second wins")[0][0] == 1
    m.close()


def test_ransac_batch_with_an_empty_set_in_the_middle_in_two_orders(flow_mod):
    sets = wi.batch_sets()
    m = flow_mod.Tvl1Flow(2, 32, 32)                                               # 11 sets through a handle of 2 pairs
    a = _run_sets(m, sets, 320, 96, 13, "batch")
    b = _run_sets(m, [sets[k] for k in wi.BATCH_ORDER], 320, 96, 13, "batch, other order")
    m.close()
    assert a[4] == (-1, 0) and a[6] == (-1, 0) and a[5][1] == 200
    assert [c for _, c in b] == [a[k][1] for k in wi.BATCH_ORDER]                  # exact inliers: the count is the set's, the winner the index's
    assert [wn for wn, _ in b] != [a[k][0] for k in wi.BATCH_ORDER]


def test_ransac_refusals_leave_the_handle_working(flow_mod):
    from video_query_algorithms_amd._lib import VqError
    s, d = wi.stride_set()
    m = flow_mod.Tvl1Flow(2, 32, 32)
    src, dst, counts = wi.pack([(s, d)], 320)

    def refused(src, dst, counts, thr=1.0, hyp=64):
        with pytest.raises(VqError):
            m.ransac_homography(src, dst, counts, thr, hyp, seed=1)
    refused(src[:, :3], dst[:, :3], np.array([3], np.int32))                        # max_points 3
    big = np.zeros((1, 8193, 2), np.float32)
    refused(big, big, np.array([10], np.int32))                                     # max_points 8193
    refused(src, dst, counts, hyp=0)
    refused(src, dst, counts, hyp=(1 << 20) + 1)
    refused(src, dst, counts, thr=0.0)
    refused(src, dst, np.array([321], np.int32))                                    # more matches than max_points
    refused(src, dst, np.array([-1], np.int32))
    assert _run_sets(m, [(s, d)], 320, 64, wi.STRIDE_SEED, "after the refusals")[0][1] == 220
    m.close()


# ---- 3. the homography warp ------------------------------------------------------------------------------------------------------

def _same_flow(a, i, b, k):
    return all(same_bits(a[key][i], b[key][k]) for key in ("u1", "u2", "flow_x", "flow_y"))


@pytest.mark.parametrize("shape", wi.WARP_SIZES, ids=lambda s: "%dx%d" % s)
def test_whole_pixel_translations_are_the_flow_of_the_shifted_frame(flow_mod, shape):
    """With den = 1 and whole offsets the fp64 -> fp32 path of homography_warp_kernel and the bilinear sampler are exact: the flow against
    the warped second frame has the bits of the flow against the frame shifted on the host.  Two matrices per batch."""
    h, w = shape
    f0, f1 = wi.warp_pair(h, w, seed=h)
    m = flow_mod.Tvl1Flow(2, h, w, nscales=3, warps=2, iterations=30)
    two0, two1 = np.stack([f0, f0]), np.stack([f1, f1])
    plain = m.flow(two0, two1)
    ident = m.flow(two0, two1, homographies=np.stack([EYE, EYE]))
    assert _same_flow(ident, 0, plain, 0) and _same_flow(ident, 1, plain, 1)
    for ta, tb in wi.translations(w):
        Hs = np.stack([wi.translation_matrix(*ta), wi.translation_matrix(*tb)])
        got = m.flow(two0, two1, homographies=Hs)
        want = m.flow(two0, np.stack([wi.shift_replicated(f1, *ta), wi.shift_replicated(f1, *tb)]))
        for i, t in enumerate((ta, tb)):
            assert _same_flow(got, i, want, i), (shape, t, float(np.abs(got["u1"][i] - want["u1"][i]).max()))
        assert not _same_flow(got, 0, got, 1)
        one = m.flow(two0[:1], two1[:1], homographies=Hs[1:])                      # the second matrix alone in front
        assert _same_flow(one, 0, got, 1)
    m.close()


def test_perspective_warp_and_its_inverse_against_the_oracle(flow_mod):
    from video_query_algorithms_amd._lib import VqError
    h, w = 64, 80
    f0, f1 = wi.warp_pair(h, w, seed=9)
    Hs = np.stack([wi.H_PERSPECTIVE, np.linalg.inv(wi.H_PERSPECTIVE)])
    m = flow_mod.Tvl1Flow(2, h, w, **wi.FIXED_KW)
    r = m.flow(np.stack([f0, f0]), np.stack([f1, f1]), homographies=Hs)
    for i in range(2):
        u1, u2, _ = tv.tvl1_flow(f0, tv.warp_homography(f1, Hs[i]), **wi.FIXED_KW)
        d = max(np.abs(r["u1"][i] - u1).max(), np.abs(r["u2"][i] - u2).max())
        print("\n[warp edges] perspective matrix %d: |d| %.3g px" % (i, d))
        assert d <= wi.FIELD_BOUND, (i, d)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    with pytest.raises(VqError):
        m.flow(np.stack([f0, f0]), np.stack([f1, f1]), homographies=np.stack([Hs[0], singular]))
    again = m.flow(np.stack([f0, f0]), np.stack([f1, f1]), homographies=Hs)
    m.close()
    assert _same_flow(again, 0, r, 0) and _same_flow(again, 1, r, 1)


# ---- 4. vq_flow_warped: guards, fallbacks, alignment in a batch ----------------------------------------------------------------------

SEED = 3


@pytest.fixture(scope="module")
def guarded(flow_mod):
    """The batch (a, b, c, d) and the batch (b, c, a, d) through one handle of four pairs at 100 x 141."""
    h, w = wi.GUARD_SIZE
    m = flow_mod.Tvl1Flow(4, h, w)
    out = {}
    for order in ("abcd", "bcad"):
        f0, f1 = wi.guard_batch(order)
        out[order] = {"f0": f0, "f1": f1, "warped": m.warped(f0, f1, seed=SEED, images=True, fields=True), "plain": m.flow(f0, f1)}
    f0, f1 = wi.guard_batch("abcd")
    out["steps"] = m.warped_steps(f0, f1, seed=SEED, images=True, fields=True)
    out["solo"] = m.warped(f0[:1], f1[:1], seed=SEED, images=True, fields=True)
    m.close()
    return out


@pytest.mark.parametrize("order", ["abcd", "bcad"])
def test_warped_guards_and_identity_fallback(guarded, order):
    g = guarded[order]
    r, plain = g["warped"], g["plain"]
    for p, name in enumerate(order):
        assert r["matches"][p] == len(wi.oracle_corners(g["f0"][p])), (name, int(r["matches"][p]))
        is_identity = bool((r["H"][p] == EYE).all())
        assert is_identity == bool(r["matches"][p] <= 50 or r["inliers"][p] <= 25), (name, int(r["matches"][p]), int(r["inliers"][p]), r["H"][p])
        if is_identity:                                                            # the identity warp is exact: weights 0 and 1
            assert _same_flow(r, p, plain, p), (name, float(np.abs(r["u1"][p] - plain["u1"][p]).max()))
    a, b, c = order.index("a"), order.index("b"), order.index("c")
    assert (r["H"][b] == EYE).all() and r["matches"][b] == 0 and r["inliers"][b] == 0 and (r["u1"][b] == 0).all()
    assert (r["H"][c] == EYE).all() and r["matches"][c] == 50
    assert r["inliers"][c] > 25                                                    # 50 matches alone keep pair (c) on the identity
    assert not (r["H"][a] == EYE).all() and r["matches"][a] > 50 and r["inliers"][a] > 25
    # pair (a): the oracle's estimate from the device's own first-pass flow, hashed with the pair's index in THIS batch
    G, matches, inliers = wo.camera_motion(g["f0"][a], plain["u1"][a], plain["u2"][a], seed=SEED, pair=a)
    assert (matches, inliers) == (int(r["matches"][a]), int(r["inliers"][a]))
    assert np.abs(G - r["H"][a]).max() <= 1e-8 * np.abs(G).max(), np.abs(G - r["H"][a]).max()
    assert np.abs(r["H"][a] - wi.H_MILD).max() < 0.5


def test_warped_pairs_keep_their_results_when_the_batch_is_reordered(guarded):
    """(a, b, c, d) against (b, c, a, d): the first pass and the corner count of a pair are its own wherever it rides (the p = i /
    max_corners indexing of move_corners_kernel); the pairs on the identity fallback give the same bits in both places."""
    first, third = guarded["abcd"], guarded["bcad"]
    for k in "abcd":
        i, j = "abcd".index(k), "bcad".index(k)
        assert first["warped"]["matches"][i] == third["warped"]["matches"][j], k
        assert _same_flow(first["plain"], i, third["plain"], j), k
        if k in "bc":
            assert _same_flow(first["warped"], i, third["warped"], j), k


def test_warped_equals_its_steps_and_a_batch_of_one(guarded):
    a, b, solo = guarded["abcd"]["warped"], guarded["steps"], guarded["solo"]
    assert (a["matches"] == b["matches"]).all() and (a["inliers"] == b["inliers"]).all()
    assert np.abs(a["H"] - b["H"]).max() <= 1e-9 * np.abs(b["H"]).max()
    du = max(np.abs(a["u1"] - b["u1"]).max(), np.abs(a["u2"] - b["u2"]).max())
    d = np.abs(a["flow_x"].astype(int) - b["flow_x"].astype(int))
    print("\n[warp edges] one call against its steps: fields %.3g px, images max %d, share %.2g" % (du, d.max(), (d > 0).mean()))
    assert du <= 1e-3
    assert d.max() <= 1 and (d > 0).mean() < 0.001
    assert same_bits(solo["flow_x"][0], a["flow_x"][0]) and same_bits(solo["flow_y"][0], a["flow_y"][0])
    assert same_bits(solo["u1"][0], a["u1"][0]) and same_bits(solo["u2"][0], a["u2"][0]) and same_bits(solo["H"][0], a["H"][0])
