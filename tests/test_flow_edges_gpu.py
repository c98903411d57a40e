"""GPU: the TV-L1 tile kernel, its host schedule and the camera-motion kernels (csrc/vq_flow.hip) where the end-to-end tests of
tests/test_flow_gpu.py and tests/test_warp_gpu.py do not look: the stopping rule held EXACTLY (a replayed block against a direct run of
the same count, bit for bit; the oracle forced to the device's schedule at the fixed-count bound; every stop decision audited against
the oracle's fp64 error trace), every class of tile cut named by the library (vq_flow_tile_cut) and run, hard inputs (flat, saturated,
step edges, whole-pixel noise, brightness change, flow out of the frame, occlusion: tests/_flow_inputs.py), every parameter varied, the
device-pointer / stream entry, reused handles, degenerate corner frames and match sets.

PARITY UNPINNED with respect to the reference (third-party extract_warp_gpu, absent): oracle/tvl1_oracle.py and oracle/warp_oracle.py
are the only yardstick here, never the library itself.  Bounds: two device runs -- the same bits; device against oracle with the same
iteration counts (fixed by epsilon = 0, or forced on the oracle) -- 1e-4 px, the bound of tests/test_flow_gpu.py; corners bit for bit;
RANSAC winner / count / mask equal, matrix to 1e-9 relative.

Measured on an MI355X (256 compute units), printed by the tests themselves (run with -s):
    fixed counts (c), (d): largest field difference  0 px -- each of the 31 compared pairs equals the oracle bit for bit
    forced schedules (b):  largest field difference  0 px over 7 pairs of 477 to 1 153 inner iterations each (so the 1e-4 bound
                                                     holds over the long default runs and the grazing band 4 d / epsilon is empty)
    decisions audited / exempted as grazing:         6 052 / 0
    distinct cuts exercised by (a):                  77 (nx, ny, tw, th, ew, eh) in 50 runs, 61 distinct (tw, th), from 125 x 2 tiles of
                                                     8 x 8 to 21 x 1 tiles of 24 x 48; every class the test asks for
    iterations of the six pairs of the replay test:  1, 40, 43, 38, 41, 48 (the cap)
    wall time of this module:                        18.0 s in the tests, 20.1 s for pytest (21.7 s with the interpreter's start)
    tests/test_flow_gpu.py + tests/test_warp_gpu.py: 5.4 s for pytest (7.0 s with the start) in their form at the parent commit, run
                                                     in the same session on this library, whose kernels are the parent's; 5.6 s (7.4 s)
                                                     with the added batch of test_blocked_tiles_against_the_oracle_on_every_cut
"""
import time

import numpy as np
import pytest

import _flow_inputs as fi
import tvl1_oracle as tv
import warp_oracle as wo
from test_warp_oracle import analytic_pair, synthetic_matches

pytestmark = pytest.mark.gpu

TILE_CELLS = 2048            # cells of the largest tile: 4 per thread of a 512-thread workgroup (csrc/vq_flow.hip: kTileCells)
P_DEFAULT, P_SOFT, P_STIFF = (0.25, 0.15, 0.3), (0.125, 0.05, 0.5), (0.25, 1.0, 0.1)          # (tau, lambda, theta)
RECORD = {"fixed": 0.0, "forced": 0.0, "decisions": 0, "exempt": 0}


@pytest.fixture(scope="module")
def flow_mod(gpu):
    from video_query_algorithms_amd.tsn import flow
    t0 = time.time()
    yield flow
    print("\n[flow edges] fixed-count max |d| %.3g px; forced-schedule max |d| %.3g px; decisions %d, exempted %d; module wall time %.1f s"
          % (RECORD["fixed"], RECORD["forced"], RECORD["decisions"], RECORD["exempt"], time.time() - t0))


def _flow(flow_mod, f0, f1, max_pairs=None, homographies=None, **params):
    m = flow_mod.Tvl1Flow(max_pairs or len(f0), f0.shape[1], f0.shape[2], **params)
    try:
        return m.flow(f0, f1, homographies=homographies, iterations=True)
    finally:
        m.close()


def _same_result(a, b, pairs_a=slice(None), pairs_b=slice(None)):
    return all(fi.same_bits(a[k][pairs_a], b[k][pairs_b]) for k in ("u1", "u2", "flow_x", "flow_y")) and \
        fi.same_bits(np.ascontiguousarray(a["iters"][:, :, pairs_a]), np.ascontiguousarray(b["iters"][:, :, pairs_b]))


# ---- (a) the cut never changes a bit, on cuts the test can name --------------------------------------------------------------------

def _cut_classes(cut, level, n, slots):
    nx, ny, tw, th, ew, eh = cut
    lh, lw = level
    assert nx * tw >= lw and ny * th >= lh and (nx - 1) * tw < lw and (ny - 1) * th < lh and (ew, eh) == (tw + 8, th + 8) and ew * eh <= TILE_CELLS
    tags = set()
    if nx == 1:
        tags.add("one tile column")
    if ny == 1:
        tags.add("one tile row")
    if nx * tw > lw and ny * th > lh:
        tags.add("last tile partly outside")
    if ew > 64:
        tags.add("tile wider than 64 cells")
    if ew * eh > TILE_CELLS - ew:
        tags.add("tile within one row of full")
    if nx * ny * n > slots:
        tags.add("more than one round")
    return tags


def _choose_counts(cuts, tags):
    """Pair counts to run, from cuts[n] (the cut of every level for n pairs) and tags[n] (its classes): 1, then the smallest count
    that brings each class not seen yet, then the smallest counts with a cut list not chosen yet until three lists differ."""
    chosen = [1]
    for n in sorted(cuts):
        if tags[n] - set().union(*[tags[k] for k in chosen]):
            chosen.append(n)
    for n in sorted(cuts):
        if len({tuple(cuts[k]) for k in chosen}) < 3 and tuple(cuts[n]) not in {tuple(cuts[k]) for k in chosen}:
            chosen.append(n)
    return chosen


def test_cut_invariance_on_named_cuts(flow_mod):
    """A pair's fields do not depend on how its levels are cut into tiles.  The cut follows the level size, the number of pairs in the
    batch and the compute units; Tvl1Flow.tile_cuts names it, so the pair counts are CHOSEN for their cuts: per shape the counts that
    bring a class of cut not seen yet, and at least two counts whose cuts differ.  The target pair rides last in every batch."""
    import torch
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    seen_tags, seen_cuts = set(), set()
    runs = 0
    for (h, w, scales, most) in ((64, 80, 3, 32), (131, 174, 3, 32), (256, 340, 5, 32), (48, 500, 5, 32), (500, 48, 5, 32), (480, 854, 2, 8),
                                 (16, 1000, 1, 32)):
        fill = [fi.shifted_pair(h, w, 1.0, 0.5, seed=40), fi.noise_band(h, w, seed=41), fi.identical(h, w, seed=42)]
        for target, iters, warps in ((fi.hard_pair(h, w, seed=43), 6, 2), (fi.shifted_pair(h, w, -2.25, 1.5, seed=44), 8, 1)):
            m = flow_mod.Tvl1Flow(most, h, w, epsilon=0.0, iterations=iters, warps=warps, nscales=scales)
            assert m.levels == tv.pyramid_sizes(h, w, scales)
            cuts = {n: m.tile_cuts(n) for n in range(1, most + 1)}
            tags = {n: set().union(*[_cut_classes(c, lvl, n, slots) for c, lvl in zip(cuts[n], m.levels)]) for n in cuts}
            chosen = _choose_counts(cuts, tags)
            assert len({tuple(cuts[k]) for k in chosen}) >= 2, (h, w, "every pair count up to %d gives the same cut" % most)
            results = []
            for n in chosen:
                batch = [fill[k % 3] for k in range(n - 1)] + [target]
                f0, f1 = fi.stack(batch)
                r = m.flow(f0, f1, images=False, iterations=True)
                runs += 1
                assert np.isfinite(r["u1"]).all() and (r["iters"][:, :, -1] == iters).all()
                results.append(r)
                seen_tags |= tags[n]
                seen_cuts |= set(cuts[n])
            for n, r in zip(chosen[1:], results[1:]):
                assert fi.same_bits(r["u1"][-1], results[0]["u1"][0]) and fi.same_bits(r["u2"][-1], results[0]["u2"][0]), \
                    (h, w, "the target pair alone and last of %d" % n, cuts[1], cuts[n])
            m.close()
    print("\n[flow edges] (a) %d runs, %d distinct cuts, %d distinct (tw, th): %s" % (runs, len(seen_cuts), len({c[2:4] for c in seen_cuts}),
                                                                                   sorted(seen_cuts)))
    want = {"one tile column", "one tile row", "last tile partly outside", "tile wider than 64 cells", "tile within one row of full", "more than one round"}
    assert want <= seen_tags, sorted(want - seen_tags)
    assert len({c[2:4] for c in seen_cuts}) >= 6


# ---- (b) the stopping rule, exactly ------------------------------------------------------------------------------------------------

def test_replayed_block_equals_the_direct_run_bit_for_bit(flow_mod):
    """One level, one warp, the convergence test active, six different pairs in one batch: they stop in different launches, in either
    set of planes, inside a block (replayed with exactly j + 1 iterations) or at its end, and one at the cap.  Each pair alone with
    epsilon = 0 and its own count as the cap runs the same iterations without any stop decision: the same bits."""
    h, w, cap = 64, 80, 48
    pairs = [fi.identical(h, w, seed=1), fi.square_on_black(h, w, seed=1), fi.noise_band(h, w, seed=2), fi.brightness_band(h, w, seed=1),
             fi.checkerboard(h, w, seed=2), fi.hard_pair(h, w, seed=1)]
    f0, f1 = fi.stack(pairs)
    r = _flow(flow_mod, f0, f1, nscales=1, warps=1, iterations=cap)
    k = [int(v) for v in r["iters"][0, 0]]
    print("\n[flow edges] (b) iterations of the batch:", k)
    assert k[0] == 1 and max(k) == cap and all(1 <= v <= cap for v in k)
    assert {v % 4 for v in k} == {0, 1, 2, 3}, k                          # stops at every place of a block of 4
    assert {((v + 3) // 4) % 2 for v in k} == {0, 1}, k                   # ... after an odd and an even number of blocks: either set
    for p, kp in enumerate(k):
        solo = _flow(flow_mod, f0[p:p + 1], f1[p:p + 1], nscales=1, warps=1, epsilon=0.0, iterations=kp)
        assert int(solo["iters"][0, 0, 0]) == kp
        assert _same_result(solo, r, slice(0, 1), slice(p, p + 1)), "pair %d: stopped at %d, differs from the direct run of %d iterations" % (p, kp, kp)


def test_forced_schedule_oracle_and_audit_of_every_stop_decision(flow_mod):
    """Default parameters (5 scales, 5 warps, epsilon 0.01, up to 300 iterations).  The oracle runs the DEVICE's iteration counts
    (schedule=): both now do the same operations, so the fixed-count bound of 1e-4 px holds where the rule-against-rule comparison of
    tests/test_flow_gpu.py needs 2e-2.  The oracle's fp64 trace of that run then judges every decision the device took (audit_decisions:
    go on above eps^2, stop at or below it or at the cap; exempt only within 4 d / epsilon of the threshold, d = the pair's measured
    field difference; at most 5 % of all decisions exempt)."""
    motions = [(3.0, -1.5), (-6.5, 2.0), (0.4, 0.3), (4.0, -3.0)]
    batches = [[fi.shifted_pair(256, 340, dx, dy, seed=10 + k, margin=40) for k, (dx, dy) in enumerate(motions)],
               [fi.hard_pair(96, 128, seed=s) for s in (1, 2, 3)]]
    decisions = exempt = 0
    for pairs in batches:
        f0, f1 = fi.stack(pairs)
        r = _flow(flow_mod, f0, f1)
        assert r["iters"].shape[:2] == (5, 5) and r["iters"].min() >= 1 and r["iters"].max() <= tv.ITERATIONS
        for p in range(len(pairs)):
            counts = [[int(v) for v in lvl] for lvl in r["iters"][:, :, p]]
            u1, u2, ran, trace = tv.tvl1_flow(f0[p], f1[p], schedule=counts, trace=True)
            assert ran == counts
            d = fi.field_difference(r["u1"][p], r["u2"][p], u1, u2)
            print("\n[flow edges] (b) %s pair %d: %d iterations, |d| %.3g px" % (f0.shape[1:], p, sum(map(sum, counts)), d))
            RECORD["forced"] = max(RECORD["forced"], d)
            fi.assert_fields_match(r["u1"][p], r["u2"][p], u1, u2, "pair %d of %s against the oracle on the device's schedule" % (p, f0.shape[1:]))
            assert (r["flow_x"][p] == tv.flow_to_image(r["u1"][p])).all() and (r["flow_y"][p] == tv.flow_to_image(r["u2"][p])).all()
            n, e = fi.audit_decisions(counts, trace, tv.EPSILON, tv.ITERATIONS, d)
            decisions += n
            exempt += e
    RECORD["decisions"], RECORD["exempt"] = decisions, exempt
    print("\n[flow edges] (b) decisions audited %d, exempted as grazing %d" % (decisions, exempt))
    assert decisions > 2000 and exempt <= 0.05 * decisions


# ---- (c) hard inputs and parameters at fixed counts --------------------------------------------------------------------------------

# kinds: "h" = a hard pair, "s" = a smooth one, both in one batch where the numpy oracle is cheap.  The 480 x 854 entries run ONE kind
# each and 720 x 1280 one hard pair, one warp, three iterations, on purpose: there the oracle is the cost of the test.
FIXED = [  # h, w, iterations, warps, nscales asked, scale_step, (tau, lambda, theta), bound, kinds
    (16, 16, 1, 1, 1, 0.8, P_DEFAULT, 20.0, "hs"), (16, 16, 5, 3, 8, 0.95, P_DEFAULT, 5.0, "hs"),
    (17, 19, 2, 3, 8, 0.95, P_SOFT, 64.0, "hs"), (17, 19, 13, 1, 2, 0.5, P_STIFF, 20.0, "hs"),
    (16, 1000, 3, 1, 3, 0.8, P_DEFAULT, 20.0, "hs"), (16, 1000, 4, 3, 1, 0.8, P_SOFT, 5.0, "hs"),
    (1000, 16, 5, 1, 1, 0.8, P_STIFF, 5.0, "hs"), (1000, 16, 8, 1, 2, 0.95, P_SOFT, 64.0, "hs"),
    (131, 174, 13, 3, 8, 0.8, P_DEFAULT, 20.0, "hs"), (131, 174, 4, 1, 8, 0.5, P_SOFT, 64.0, "hs"),
    (131, 174, 8, 3, 5, 0.95, P_STIFF, 5.0, "hs"), (131, 174, 1, 3, 3, 0.8, P_DEFAULT, 20.0, "hs"),
    (131, 174, 2, 1, 3, 0.8, P_STIFF, 64.0, "hs"), (131, 174, 3, 1, 2, 0.8, P_SOFT, 20.0, "hs"),
    (480, 854, 5, 1, 2, 0.8, P_DEFAULT, 20.0, "h"), (480, 854, 3, 3, 3, 0.5, P_SOFT, 64.0, "s"),
    (720, 1280, 3, 1, 1, 0.8, P_DEFAULT, 20.0, "h"),
]


def test_fixed_configurations_cover_what_the_issue_lists():
    assert {c[2] for c in FIXED} == {1, 2, 3, 4, 5, 8, 13} and {c[3] for c in FIXED} == {1, 3}
    assert {c[5] for c in FIXED} == {0.5, 0.8, 0.95} and {c[6] for c in FIXED} == {P_DEFAULT, P_SOFT, P_STIFF} and {c[7] for c in FIXED} == {20.0, 5.0, 64.0}
    assert {(16, 16), (16, 1000), (1000, 16), (17, 19), (131, 174), (480, 854), (720, 1280)} == {c[:2] for c in FIXED}
    levels = {len(tv.pyramid_sizes(c[0], c[1], c[4], c[5])) for c in FIXED}
    assert 1 in levels and 8 in levels and any(len(tv.pyramid_sizes(c[0], c[1], c[4], c[5])) < c[4] for c in FIXED)        # asked for 8, got fewer
    assert sum(1 for c in FIXED if c[:2] == (720, 1280)) == 1


@pytest.mark.parametrize("cfg", FIXED, ids=lambda c: "%dx%d-i%d-w%d-s%d-%g-t%g" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6][2]))
def test_hard_inputs_and_parameters_at_fixed_counts(flow_mod, cfg):
    h, w, iters, warps, scales, step, (tau, lam, theta), bound, kinds = cfg
    pairs = [fi.hard_pair(h, w, seed=h + iters) if k == "h" else fi.shifted_pair(h, w, 1.75, -0.5, seed=w + iters) for k in kinds]
    f0, f1 = fi.stack(pairs)
    m = flow_mod.Tvl1Flow(len(pairs), h, w, epsilon=0.0, iterations=iters, warps=warps, nscales=scales, scale_step=step, tau=tau, lambda_=lam,
                          theta=theta, bound=bound)
    assert m.levels == tv.pyramid_sizes(h, w, scales, step)
    r = m.flow(f0, f1, iterations=True)
    m.close()
    for p, kind in enumerate(kinds):
        cc = np.zeros(4, np.int64)
        u1, u2, counts = tv.tvl1_flow(f0[p], f1[p], nscales=scales, warps=warps, iterations=iters, epsilon=0.0, scale_step=step, tau=tau, lam=lam,
                                      theta=theta, case_counts=cc)
        assert np.isfinite(r["u1"][p]).all() and np.isfinite(r["u2"][p]).all()
        d = fi.assert_fields_match(r["u1"][p], r["u2"][p], u1, u2, "%s pair of %s" % (kind, (cfg,)))
        RECORD["fixed"] = max(RECORD["fixed"], d)
        print("\n[flow edges] (c) %s %s: |d| %.3g px, cases %s" % (cfg, kind, d, cc.tolist()))
        assert (r["flow_x"][p] == tv.flow_to_image(r["u1"][p], bound)).all() and (r["flow_y"][p] == tv.flow_to_image(r["u2"][p], bound)).all()
        assert (r["iters"][:, :, p] == iters).all() and (np.array(counts) == iters).all()


def test_hard_inputs_reach_every_case_of_the_thresholding_step():
    """Oracle side only: over the hard pairs of FIXED up to 131 x 174 (the ones cheap for numpy) cells fall into each of the four cases of
    the thresholding step -- below, above, between with a gradient, between without one -- so the runs above did exercise all four."""
    cases = np.zeros(4, np.int64)
    for (h, w, iters, warps, scales, step, (tau, lam, theta), _, kinds) in FIXED:
        if "h" in kinds and h * w <= 131 * 174:
            cases += fi.case_counts(*fi.hard_pair(h, w, seed=h + iters), nscales=scales, warps=warps, iterations=iters, epsilon=0.0, scale_step=step,
                                    tau=tau, lam=lam, theta=theta)
    print("\n[flow edges] (c) cells per case over the hard pairs:", cases.tolist())
    assert (cases > 0).all(), cases.tolist()


# ---- (d) entry paths and handle state ----------------------------------------------------------------------------------------------

def test_host_pointers_device_pointers_on_a_stream_and_a_larger_handle_give_the_same_bits(flow_mod):
    import ctypes as C
    import torch
    from video_query_algorithms_amd import _lib
    _lib.require_torch_runtime("this test")
    h, w = 96, 128
    f0, f1 = fi.stack([fi.hard_pair(h, w, seed=5), fi.shifted_pair(h, w, 2.0, -1.0, seed=6), fi.leaving(h, w, seed=7)])
    n = len(f0)
    host = _flow(flow_mod, f0, f1)
    assert len(set(host["iters"].ravel().tolist())) > 5                  # the stop rule is at work
    roomy = _flow(flow_mod, f0, f1, max_pairs=8)
    assert _same_result(host, roomy), "a handle with max_pairs 8 differs from one with max_pairs 3"
    m = flow_mod.Tvl1Flow(n, h, w)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t0, t1 = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    stream.synchronize()
    dev = {"u1": np.empty((n, h, w), np.float32), "u2": np.empty((n, h, w), np.float32), "flow_x": np.empty((n, h, w), np.uint8),
           "flow_y": np.empty((n, h, w), np.uint8), "iters": np.zeros((len(m.levels), m.params.warps, n), np.int32)}
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in dev.items()}
    assert stream.cuda_stream != 0
    _lib.call("vq_flow_tvl1", m._h, t0.data_ptr(), t1.data_ptr(), 1, n, None, ptr["u1"], ptr["u2"], ptr["flow_x"], ptr["flow_y"], ptr["iters"],
              stream.cuda_stream)
    m.close()
    assert _same_result(host, dev), "device pointers on a stream differ from host pointers"
    assert (t0.cpu().numpy() == f0).all() and (t1.cpu().numpy() == f1).all()           # the caller's frames are inputs only


def test_reused_handle_equals_fresh_handles(flow_mod):
    """n = max, then n = 1, then n = max on other frames through ONE handle: what the earlier calls leave behind (per-pair state, the
    live flag in pinned memory, the second set of planes, fields of pairs beyond n) changes nothing."""
    h, w = 96, 128
    a = fi.stack([fi.hard_pair(h, w, seed=8), fi.shifted_pair(h, w, -3.0, 1.0, seed=9), fi.noise_band(h, w, seed=10), fi.identical(h, w, seed=11)])
    b = fi.stack([fi.square_on_black(h, w, seed=12)])
    c = fi.stack([fi.identical(h, w, seed=13), fi.leaving(h, w, seed=14), fi.hard_pair(h, w, seed=15), fi.checkerboard(h, w, seed=16)])
    m = flow_mod.Tvl1Flow(4, h, w)
    reused = [m.flow(f0, f1, iterations=True) for f0, f1 in (a, b, c)]
    m.close()
    for k, (f0, f1) in enumerate((a, b, c)):
        assert _same_result(reused[k], _flow(flow_mod, f0, f1, max_pairs=4)), "call %d of a reused handle differs from a fresh handle" % k
    assert (reused[2]["iters"][:, :, 0] == 1).all() and (reused[2]["u1"][0] == 0).all()


def test_perspective_homography_out_of_bounds_and_a_singular_one(flow_mod):
    h, w = 96, 128
    f0, f1 = fi.shifted_pair(h, w, 2.0, 1.0, seed=17, margin=32)
    H = np.array([[1.02, 0.03, -6.0], [-0.02, 0.98, 5.0], [2e-4, -1e-4, 1.0]])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    Hi = np.linalg.inv(H)
    den = Hi[2, 0] * xs + Hi[2, 1] * ys + Hi[2, 2]
    sx, sy = (Hi[0, 0] * xs + Hi[0, 1] * ys + Hi[0, 2]) / den, (Hi[1, 0] * xs + Hi[1, 1] * ys + Hi[1, 2]) / den
    outside = (sx < 0) | (sx > w - 1) | (sy < 0) | (sy > h - 1)
    assert 0.02 < outside.mean() < 0.5 and abs(Hi[2, 0]) > 1e-5                      # part of the frame samples beyond the border
    kw = dict(nscales=3, warps=2, iterations=10, epsilon=0.0)
    r = _flow(flow_mod, f0[None], f1[None], homographies=H[None], **kw)
    u1, u2, _ = tv.tvl1_flow(f0, tv.warp_homography(f1, H), **kw)
    d = fi.assert_fields_match(r["u1"][0], r["u2"][0], u1, u2, "perspective homography")
    RECORD["fixed"] = max(RECORD["fixed"], d)
    print("\n[flow edges] (d) perspective homography: |d| %.3g px" % d)
    from video_query_algorithms_amd._lib import VqError
    m = flow_mod.Tvl1Flow(2, h, w, **kw)
    singular = np.stack([np.eye(3), np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])])
    with pytest.raises(VqError, match="singular"):
        m.flow(np.stack([f0, f0]), np.stack([f1, f1]), homographies=singular)
    with pytest.raises(VqError, match="singular"):
        m.flow(f0[None], f1[None], homographies=np.zeros((1, 3, 3)))
    again = m.flow(f0[None], f1[None], homographies=H[None], iterations=True)          # refused, not broken: the handle still works
    m.close()
    assert _same_result(again, r)


# ---- (e) corners and RANSAC --------------------------------------------------------------------------------------------------------

def _board(h, w, cy, cx):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((((ys // cy) + (xs // cx)) % 2) * 200).astype(np.uint8)          # periodic, free of noise: exact strength ties


@pytest.mark.parametrize("shape", [(17, 19), (49, 67), (256, 340), (480, 854)], ids=lambda s: "%dx%d" % s)
def test_corners_bit_for_bit_on_ties_block_tails_and_mixed_batches(flow_mod, shape):
    h, w = shape
    rng = np.random.default_rng(h)
    cy, cx = (4, 5) if h < 100 else (12, 16)
    busy = rng.integers(0, 256, (h, w), dtype=np.uint8) if h <= 256 else analytic_pair(h, w, np.eye(3), seed=3)[0]
    frames = np.stack([np.full((h, w), 77, np.uint8), busy, _board(h, w, cy, cx), np.zeros((h, w), np.uint8), _board(h, w, cx, cy)])
    assert ((h * w) % 256 == 0) == (shape == (256, 340))                           # elsewhere the last block of a frame is partly outside it
    m = flow_mod.Tvl1Flow(len(frames), h, w)
    peaks = wo.corner_peaks(wo.corner_strength(frames[2]))
    values = peaks[peaks > 0]
    assert len(values) > len(np.unique(values))                                    # the board does have exact ties
    for cap, q, md in ((1000, 0.001, 3.0), (7, 0.01, 3.0), (1000, 0.05, 0.0)):
        corners, counts = m.good_features(frames, cap, q, md)
        for i in range(len(frames)):
            want = wo.good_features(frames[i], cap, q, md)
            assert counts[i] == len(want), (shape, i, cap, q, md, counts[i], len(want))
            assert fi.same_bits(corners[i, :counts[i]], want), (shape, i, cap, q, md)
            assert (corners[i, counts[i]:] == 0).all()
        assert counts[0] == 0 and counts[3] == 0                                   # constant frames beside busy ones: no maximum leaks across
        if cap == 7:
            assert counts[1] == 7 and counts[2] == 7                               # the cap is smaller than the number of peaks
    solo, c1 = m.good_features(frames[2:3])
    both, c2 = m.good_features(frames)
    assert c1[0] == c2[2] and fi.same_bits(solo[0], both[2])
    m.close()


def _ransac_sets():
    H = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [2e-5, -1e-5, 1.0]])
    full = synthetic_matches(H, 220, 90, seed=5)[:2]
    t = np.arange(40, dtype=np.float32)
    line = np.stack([2 * t, 3 * t + 7], 1).astype(np.float32)
    same = np.tile(np.float32([[31.5, 40.25]]), (40, 1))
    four = np.float32([[10, 12], [200, 20], [190, 170], [15, 160]])
    p = np.c_[four, np.ones(4)] @ H.T
    empty = np.zeros((0, 2), np.float32)
    return {"full": full, "three": (full[0][:3], full[1][:3]), "none": (empty, empty), "identical": (same, same + np.float32(2.0)),
            "collinear": (line, line + np.float32([1.0, -2.0])), "four": (four, (p[:, :2] / p[:, 2:]).astype(np.float32)),
            "full again": synthetic_matches(H, 150, 60, seed=9, noise=0.1)[:2]}


def _pack(sets, names, mp):
    src, dst = np.zeros((len(names), mp, 2), np.float32), np.zeros((len(names), mp, 2), np.float32)
    counts = np.array([len(sets[k][0]) for k in names], np.int32)
    for i, k in enumerate(names):
        src[i, :counts[i]], dst[i, :counts[i]] = sets[k]
    return src, dst, counts


@pytest.mark.parametrize("mp,hyp", [(320, 40), (320, 3000), (8192, 96)], ids=["40-hypotheses", "3000-hypotheses", "8192-points"])
def test_ransac_on_degenerate_sets_equals_the_oracle(flow_mod, mp, hyp):
    """Fewer than 4 matches, none at all beside a full set, all matches identical, all collinear, exactly 4, the largest max_points
    (128 KB of dynamic LDS) with a few hundred real matches, more sets in one call than the handle has pairs, hypotheses below and far
    above the 256 threads of a workgroup.  Where nothing can be drawn the answer is the oracle's: identity, 0 inliers, winner -1."""
    sets = _ransac_sets()
    names = ["none", "full", "three", "identical", "collinear", "four", "full again"]
    src, dst, counts = _pack(sets, names, mp)
    m = flow_mod.Tvl1Flow(2, 32, 32)                                               # 7 sets through a handle of 2 pairs
    for refit in (False, True):
        r = m.ransac_homography(src, dst, counts, 1.0, hyp, seed=21, refit=refit)
        for i, k in enumerate(names):
            G, cnt, winner, mask = wo.ransac_homography(sets[k][0], sets[k][1], 1.0, hyp, seed=21, pair=i, refit=refit)
            assert (int(r["winner"][i]), int(r["inliers"][i])) == (winner, cnt), (k, refit, r["winner"][i], r["inliers"][i], winner, cnt)
            assert (r["mask"][i, :counts[i]] == mask).all() and r["mask"][i, counts[i]:].sum() == 0, (k, refit)
            assert np.abs(r["H"][i] - G).max() <= 1e-9 * np.abs(G).max(), (k, refit, np.abs(r["H"][i] - G).max())
            if k in ("none", "three", "identical", "collinear"):
                assert winner == -1 and cnt == 0 and (r["H"][i] == np.eye(3)).all(), k
        assert r["inliers"][1] >= 220 and r["inliers"][5] == 4 and r["inliers"][6] >= 100
    m.close()
