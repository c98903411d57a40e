"""Inputs and runs of the flow handle whose results are pinned as sha256 hashes in tests/golden/flow_plan/parent_bits.json: the bits the
library gave BEFORE its host half was reorganised (tools/flow_record_bits.py records them, tests/test_flow_bits_gpu.py compares).
Every case is a function of the flow module (video_query_algorithms_amd.tsn.flow) that returns name -> array; arrays are hashed as
their bytes, so a float field is compared as its bit patterns and H as the bytes of its doubles."""
import hashlib

import numpy as np

import _flow_inputs as fi
import _warp_inputs as wi

CUT_SHAPES = ((64, 80, 3), (131, 174, 3), (256, 340, 5), (48, 500, 5), (500, 48, 5), (480, 854, 2), (16, 1000, 1))         # h, w, scales
FLOW_KEYS = ("u1", "u2", "flow_x", "flow_y", "iters")
WARPED_KEYS = ("u1", "u2", "flow_x", "flow_y", "H", "matches", "inliers")


def ragged_pairs():
    """3 pairs of 61 x 83: levels of odd sizes, 9 iterations (no multiple of the block of 4)."""
    return fi.stack([fi.shifted_pair(61, 83, 1.5, -0.75, seed=61 + k, margin=8) for k in range(3)])


def ragged_handle(flow):
    return flow.Tvl1Flow(4, 61, 83, epsilon=0.0, iterations=9, warps=2, nscales=3)


def case_a(flow):
    m = ragged_handle(flow)
    try:
        r = m.flow(*ragged_pairs(), iterations=True)
    finally:
        m.close()
    return {k: r[k] for k in FLOW_KEYS}


def case_b(flow):
    H = np.stack([wi.H_PERSPECTIVE, wi.translation_matrix(3, -2), np.eye(3)])
    m = ragged_handle(flow)
    try:
        r = m.flow(*ragged_pairs(), homographies=H, iterations=True)
    finally:
        m.close()
    return {k: r[k] for k in FLOW_KEYS}


def stop_rule_pairs():
    """The six pairs of test_flow_edges_gpu.test_replayed_block_equals_the_direct_run_bit_for_bit."""
    h, w = 64, 80
    return fi.stack([fi.identical(h, w, seed=1), fi.square_on_black(h, w, seed=1), fi.noise_band(h, w, seed=2), fi.brightness_band(h, w, seed=1),
                     fi.checkerboard(h, w, seed=2), fi.hard_pair(h, w, seed=1)])


def case_c(flow):
    f0, f1 = stop_rule_pairs()
    m = flow.Tvl1Flow(6, 64, 80, nscales=1, warps=1, iterations=48)
    try:
        r = m.flow(f0, f1, iterations=True)
    finally:
        m.close()
    return {k: r[k] for k in FLOW_KEYS}


def case_d(flow):
    f0, f1 = wi.guard_batch("abcd")
    m = flow.Tvl1Flow(4, *wi.GUARD_SIZE)
    try:
        r = m.warped(f0, f1, seed=3, images=True, fields=True)
    finally:
        m.close()
    return {k: r[k] for k in WARPED_KEYS}


def case_e_corners(flow):
    frames = np.stack(list(wi.small_frames(37, 53).values()))
    m = flow.Tvl1Flow(len(frames), 37, 53)
    try:
        corners, counts = m.good_features(frames)
    finally:
        m.close()
    return {"corners": corners, "counts": counts}


def case_e_ransac(flow):
    src, dst, counts = wi.pack(wi.batch_sets(), 320)
    m = flow.Tvl1Flow(2, 32, 32)
    try:
        r = m.ransac_homography(src, dst, counts, wi.THRESHOLD, 96, seed=13, refit=True)
    finally:
        m.close()
    return {k: r[k] for k in ("H", "inliers", "winner", "mask")}


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E_corners": case_e_corners, "E_ransac": case_e_ransac}
COUNT_KEYS = ("iters", "matches", "inliers", "counts", "winner")         # integer counts: recorded beside their hash where they are short


def digest(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def record(result):
    """name -> array  ->  name -> {sha256, shape, dtype[, values]} (values: the integer counts themselves, up to 64 of them)."""
    out = {}
    for k, a in result.items():
        a = np.ascontiguousarray(a)
        out[k] = {"sha256": digest(a), "shape": list(a.shape), "dtype": str(a.dtype)}
        if k in COUNT_KEYS and a.size <= 64:
            out[k]["values"] = [int(v) for v in a.reshape(-1)]
    return out


def tile_cuts(flow):
    """"h x w x scales" -> levels and [cuts of n pairs for n = 1 .. 32] on the seven shapes of test_cut_invariance_on_named_cuts."""
    out = {}
    for h, w, scales in CUT_SHAPES:
        m = flow.Tvl1Flow(32, h, w, nscales=scales)
        try:
            out["%dx%dx%d" % (h, w, scales)] = {"levels": [list(v) for v in m.levels], "cuts": [[list(c) for c in m.tile_cuts(n)] for n in range(1, 33)]}
        finally:
            m.close()
    return out
