"""CPU: the inputs of tests/_warp_inputs.py have the properties their GPU cases (tests/test_warp_edges_gpu.py) rely on, shown with
oracle/warp_oracle.py and oracle/tvl1_oracle.py alone: frame sizes that leave dead lanes in the last block of the corner kernels,
peaks next to the border, exact ties, a maximum that comes from the last block, a weak frame whose corner list a leaked maximum would
change, match sets whose RANSAC answer no rounding difference can move, translations whose warp is a whole-pixel copy, a batch that
takes every branch of the guards of the warped flow.  The helpers are controls too: each is shown the error it exists to catch."""
import numpy as np
import pytest

import _warp_inputs as wi
import tvl1_oracle as tv
import warp_oracle as wo

MARGIN = 1e-6               # no squared reprojection error of an equality case lies this close to threshold^2


# ---- corners ---------------------------------------------------------------------------------------------------------------------

def test_small_sizes_leave_the_block_tails_the_issue_names():
    tails = {s: s[0] * s[1] - wi.tail_start(*s) for s in wi.SMALL_SIZES}
    assert tails[(16, 16)] == 256 and tails[(17, 19)] == 64 + 3 and tails[(37, 53)] == 169          # one block | a wave and 3 lanes | 169 lanes
    assert all((h * w) % wi.BLOCK != 0 for h, w in wi.SMALL_SIZES[1:]) and (wi.FULL_SIZE[0] * wi.FULL_SIZE[1]) % wi.BLOCK == 0
    assert {c for c, _, _ in wi.CORNER_PARAMS} == {1, 25, 1000} and {q for _, q, _ in wi.CORNER_PARAMS} == {0.001, 0.5, 0.999}
    assert {d for _, _, d in wi.CORNER_PARAMS} == {0.0, 0.5, 1.0, 2.5, 4.5, 10.0}


def test_cached_oracle_is_the_oracle():
    for img in (wi.uniform_noise(17, 19, seed=1), wi.border_checker(16, 16), wi.flat(16, 16)):
        for cap, q, md in ((1000, 0.001, 3.0), (25, 0.5, 2.5), (1, 0.001, 0.0)):
            a, b = wi.oracle_corners(img, cap, q, md), wo.good_features(img, cap, q, md)
            assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all()
    s = wo.corner_strength(wi.uniform_noise(17, 19, seed=1))
    assert (wi.strength_and_peaks(wi.uniform_noise(17, 19, seed=1))[0] == s).all()
    # the forged maximum changes the threshold and nothing else
    img = wi.uniform_noise(17, 19, seed=1)
    assert (wi.corners_with_top(img, float(s.max())) == wo.good_features(img)).all()
    assert len(wi.corners_with_top(img, 1e3 * float(s.max()))) == 0


@pytest.mark.parametrize("shape", wi.SMALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_small_frames_have_their_properties(shape):
    h, w = shape
    fr = wi.small_frames(h, w)
    assert all(f.shape == shape and f.dtype == np.uint8 for f in fr.values())
    count = {k: len(wi.oracle_corners(f, 1000, 0.001, 0.0)) for k, f in fr.items()}
    assert count["noise"] > 10 and count["binary"] > 10 and count["flat"] == 0
    assert set(np.unique(fr["binary"])) == {0, 255}
    # binary noise and the checkerboards: exactly equal strengths among the peaks (ties in the 3 x 3 maximum and in the sort)
    for k in ("binary", "checker", "rim checker"):
        p = wi.strength_and_peaks(fr[k])[1]
        v = p[p > 0]
        assert len(v) > len(np.unique(v)) or (k == "binary" and h * w < 400), k
    # 1000 corners are more than the candidates of any small frame, 25 fewer than those of the busy ones, min_distance bites
    assert max(count.values()) < 1000 and (count["noise"] > 25 or h * w < 400)
    assert len(wi.oracle_corners(fr["noise"], 1000, 0.001, 10.0)) < len(wi.oracle_corners(fr["noise"], 1000, 0.001, 2.5)) < count["noise"]
    assert len(wi.oracle_corners(fr["noise"], 1000, 0.001, 0.5)) == count["noise"]                 # below 1 no distance is enforced
    # quality 0.999 keeps the strongest peak alone, or nothing where the frame's maximum lies on the border itself
    assert len(wi.oracle_corners(fr["noise"], 1000, 0.999, 0.0)) <= 1 and len(wi.oracle_corners(fr["noise"], 1000, 0.5, 0.0)) < count["noise"]
    # the checkerboard: its strongest peaks lie on rows / columns 1 and n - 2, and its cell edges reach rows / columns 0 and n - 1
    c = wi.oracle_corners(fr["checker"], 1000, 0.001, 0.0)
    s, p = wi.strength_and_peaks(fr["checker"])
    rim = np.zeros(shape, bool)
    rim[[1, h - 2]], rim[:, [1, w - 2]] = True, True
    assert p[rim].max() == p.max() > 0
    assert sum(1 for x, y in c if y in (1, h - 2)) > 0 and sum(1 for x, y in c if x in (1, w - 2)) > 0
    for line in (fr["checker"][0], fr["checker"][h - 1], fr["checker"][:, 0], fr["checker"][:, w - 1]):
        assert (np.diff(line.astype(int)) != 0).sum() >= 2
    assert (fr["rim checker"][0] != fr["rim checker"][1]).all() and (fr["rim checker"][:, w - 1] != fr["rim checker"][:, w - 2]).all()
    # flat except inside the last block, and the maximum comes from there
    t = fr["tail"].ravel()
    s = wi.strength_and_peaks(fr["tail"])[0]
    assert (t[:wi.tail_start(h, w)] == 90).all() and int(np.argmax(s)) >= wi.tail_start(h, w) and s.max() > 0
    assert count["tail"] > 0 or shape == (16, 300)                 # 16 x 300: the tail is part of the last row, which holds no peak
    # one bright pixel in a corner of the frame: a positive maximum on the border itself, where no peak is taken
    for k, at in (("first pixel", (0, 0)), ("last pixel", (h - 1, w - 1))):
        s = wi.strength_and_peaks(fr[k])[0]
        assert fr[k].sum() == 255 and fr[k][at] == 255 and s.max() > 0 and count[k] == 0


def test_rows_and_columns_next_to_the_border_all_carry_checkerboard_corners():
    seen = np.zeros(4, int)
    for h, w in wi.SMALL_SIZES:
        c = wi.oracle_corners(wi.border_checker(h, w), 1000, 0.001, 0.0)
        seen += [sum(1 for x, y in c if y == 1), sum(1 for x, y in c if y == h - 2), sum(1 for x, y in c if x == 1), sum(1 for x, y in c if x == w - 2)]
    assert (seen > 0).all(), seen


def test_full_frame_reaches_the_cap():
    c = wi.oracle_corners(wi.full_frame())                        # the one full-size oracle call; the GPU module reads the same list
    assert c.shape == (1000, 2)


def test_leak_batch_can_see_a_leak():
    b = wi.leak_batch()
    tops = [float(wi.strength_and_peaks(f)[0].max()) for f in b]
    assert tops[0] >= 1e3 * tops[1] > 0 and (b[0] == b[3]).all() and len(np.unique(b[1])) <= 4
    own, leaked = wi.oracle_corners(b[1]), wi.corners_with_top(b[1], tops[0])
    assert len(own) > 10 and len(leaked) != len(own)              # thresholded with the strong frame's maximum the weak frame loses its corners


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------------

def _safe(src, dst, hyp, seed, pair):
    """The robustness condition of an equality case; -> the margins, which agree with the oracle's own answer."""
    m = wi.ransac_margins(src, dst, wi.THRESHOLD, hyp, seed, pair)
    _, cnt, winner, mask = wo.ransac_homography(src, dst, wi.THRESHOLD, hyp, seed=seed, pair=pair, refit=False)
    assert (m["winner"], m["count"]) == (winner, cnt) and mask.sum() == cnt
    assert m["margin"] > MARGIN and m["clear"], m
    return m


def test_no_winner_sets_have_no_winner():
    for name, (s, d) in wi.no_winner_sets().items():
        for seed in (0, 21):
            for refit in (False, True):
                G, cnt, winner, mask = wo.ransac_homography(s, d, wi.THRESHOLD, 300, seed=seed, pair=1, refit=refit)
                assert (G == np.eye(3)).all() and cnt == 0 and winner == -1 and mask.sum() == 0 and len(mask) == len(s), name
    s, d = wi.no_winner_sets()["collinear"]
    assert len(s) == 40 and (s == np.rint(s)).all() and (d == np.rint(d)).all()
    assert all(wo._orient(s[a], s[b], s[c]) == 0.0 for a, b, c in ((0, 1, 2), (3, 17, 39), (5, 4, 30)))
    s, d = wi.no_winner_sets()["two points"]
    assert len(s) == 60 and len(np.unique(s, axis=0)) == 2
    s, d = wi.no_winner_sets()["mirrored"]
    assert len(s) == 60 and all(wo._orient(s[a], s[b], s[c]) * wo._orient(d[a], d[b], d[c]) < 0 for a, b, c in ((0, 1, 2), (3, 17, 39), (5, 4, 30)))


def test_small_full_and_stride_sets_are_safe_for_equality():
    for name, (s, d) in wi.small_sets().items():
        m = _safe(s, d, 64, 21, 0)
        assert (m["winner"], m["count"]) == (0, len(s)), name
    s, d, inl = wi.full_set()
    assert len(s) == 8192 and inl.sum() == 6000
    m = _safe(s, d, 64, 7, 0)
    assert m["count"] == 6000 and m["winner"] >= 0
    m = _safe(s[:4000], d[:4000], 64, 7, 0)
    assert m["count"] == inl[:4000].sum()
    s, d = wi.stride_set()
    for hyp in wi.STRIDE_HYPOTHESES[2:]:
        m = _safe(s, d, hyp, wi.STRIDE_SEED, 0)
        assert m["count"] == 220 and (m["ties"] >= 2 or hyp < 257), (hyp, m)      # first among equals is decided across threads
    # hypotheses 255 / 256 / 257: the 256th and 257th hypothesis exist and are valid or not -- the counts of valid ones differ
    for hyp, (none, first) in wi.FEW_SEEDS.items():
        assert _safe(s, d, hyp, none, 0)["winner"] == -1 and _safe(s, d, hyp, first, 0)["winner"] == 0
    assert _safe(s, d, 2, 1, 0)["winner"] == 1                   # ... and one where the second of two hypotheses wins


def test_batch_sets_are_safe_for_equality_in_both_orders():
    sets = wi.batch_sets()
    counts = [len(s) for s, _ in sets]
    assert len(sets) >= 9 and len(set(counts)) == len(counts) and counts[4] == 0 and 0 < counts[6] < 4
    assert sorted(wi.BATCH_ORDER) == list(range(len(sets))) and all(i != k for i, k in enumerate(wi.BATCH_ORDER))
    winners = []
    for order in (list(range(len(sets))), wi.BATCH_ORDER):
        for i, k in enumerate(order):
            winners.append((k, i, _safe(sets[k][0], sets[k][1], 96, 13, i)["winner"]))
    moved = {k: {wn for kk, _, wn in winners if kk == k} for k in range(len(sets))}
    assert sum(1 for v in moved.values() if len(v) == 2) >= 3      # the index of a set is part of its hash: other samples, another winner
    src, dst, cnt = wi.pack(sets, 320)
    assert np.isnan(src[0, cnt[0]:]).all() and np.isnan(dst[4]).all() and np.isfinite(src[5, :cnt[5]]).all()


def test_margin_helper_sees_a_grazing_match_and_a_contested_winner():
    s, d = (a.copy() for a in wi.stride_set())
    G, _, _, mask = wo.ransac_homography(s, d, wi.THRESHOLD, 64, seed=wi.STRIDE_SEED, pair=0, refit=False)
    k = int(np.flatnonzero(mask == 0)[0])
    p = G @ np.array([s[k, 0], s[k, 1], 1.0])
    d[k] = (p[:2] / p[2] + np.array([1.0, 0.0])).astype(np.float32)             # an outlier put at one threshold from its image
    assert wi.ransac_margins(s, d, wi.THRESHOLD, 64, wi.STRIDE_SEED, 0)["margin"] < 1e-3
    # two models with the same support: the winner's count does not exceed the other's
    a = wi.synthetic_matches(np.eye(3), 20, 0, seed=1)
    b = wi.synthetic_matches(wi.translation_matrix(30.0, 0.0), 20, 0, seed=2)
    m = wi.ransac_margins(np.vstack([a[0], b[0]]), np.vstack([a[1], b[1]]), wi.THRESHOLD, 200, 3, 0)
    assert m["count"] == 20 and not m["clear"]


# ---- homography warp ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", wi.WARP_SIZES, ids=lambda s: "%dx%d" % s)
def test_integer_translations_are_whole_pixel_copies(shape):
    h, w = shape
    f1 = wi.warp_pair(h, w, seed=h)[1]
    ts = [t for pair in wi.translations(w) for t in pair]
    assert {(1, 0), (-1, 0), (0, 1), (0, -1), (5, -3)} <= set(ts) and any(abs(tx) > w for tx, _ in ts)
    for tx, ty in ts:
        g1 = wi.shift_replicated(f1, tx, ty)
        want = tv.warp_homography(f1, wi.translation_matrix(tx, ty))
        assert want.dtype == np.float32 and (want == g1.astype(np.float32)).all(), (tx, ty)
        if abs(tx) > w:
            assert (g1 == f1[:, :1]).all()                        # every pixel is the replicated border
    assert (wi.shift_replicated(f1, 0, 0) == f1).all()
    g = wi.shift_replicated(f1, 5, -3)
    assert (g[:h - 3, 5:] == f1[3:, :w - 5]).all()               # content at x goes to x + t


def test_perspective_matrices_move_whole_pixels_and_leave_the_frame():
    h, w = 64, 80
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for H in (wi.H_PERSPECTIVE, np.linalg.inv(wi.H_PERSPECTIVE)):
        hi = np.linalg.inv(H)
        den = hi[2, 0] * xs + hi[2, 1] * ys + hi[2, 2]
        sx, sy = (hi[0, 0] * xs + hi[0, 1] * ys + hi[0, 2]) / den, (hi[1, 0] * xs + hi[1, 1] * ys + hi[1, 2]) / den
        assert np.abs(sx - xs).max() > 2 and np.abs(sy - ys).max() > 2 and ((sx < 0) | (sy < 0) | (sx > w - 1) | (sy > h - 1)).any()
        assert np.abs(den - 1).max() > 5e-4                       # the perspective row matters: without it pixels land elsewhere
        no_den = (hi[0, 0] * xs + hi[0, 1] * ys + hi[0, 2])
        assert np.abs(no_den - sx).max() > 0.02
        assert np.abs((H.T[0, 0] * xs + H.T[0, 1] * ys + H.T[0, 2]) - sx).max() > 1      # a transposed matrix is off by whole pixels


# ---- the guards of the warped flow -------------------------------------------------------------------------------------------------

def test_guard_batch_takes_every_branch():
    p = wi.guard_pairs()
    h, w = wi.GUARD_SIZE
    assert (h * w) % wi.BLOCK != 0 and all(f.shape == (h, w) for pair in p.values() for f in pair)
    n = {k: len(wi.oracle_corners(f0)) for k, (f0, _) in p.items()}
    assert n["a"] > wo.MIN_MATCHES and n["d"] > wo.MIN_MATCHES and n["b"] == 0
    assert n["c"] == wo.MIN_MATCHES                                # exactly at the guard: "<= 50" keeps the identity, "< 50" would not
    assert (p["b"][0] == p["b"][1]).all() and len(np.unique(p["b"][0])) == 1
    assert (p["c"][1][:, 2:] == p["c"][0][:, :-2]).all() and (p["c"][0] != p["c"][1]).any()


def test_blob_pair_would_pass_the_inlier_guard():
    """Pair (c) stays on the identity for its 50 matches alone: the oracle's flow moves its corners consistently (more than 25 inliers),
    so a matches guard that let 50 through would produce a translation."""
    f0, f1 = wi.guard_pairs()["c"]
    u1, u2, _ = tv.tvl1_flow(f0, f1, nscales=3, warps=3, iterations=60)
    c = wi.oracle_corners(f0)
    G, cnt, winner, _ = wo.ransac_homography(c, wo.matches_from_flow(c, u1, u2), seed=3, pair=2)
    assert cnt > wo.MIN_INLIERS and winner >= 0 and abs(G[0, 2] - 2.0) < 0.5 and abs(G[1, 2]) < 0.5
    H, matches, inliers = wo.camera_motion(f0, u1, u2, seed=3, pair=2)
    assert (H == np.eye(3)).all() and matches == 50
