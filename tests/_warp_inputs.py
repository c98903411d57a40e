"""Seeded inputs for the camera-motion tests (corner kernels, host selection, RANSAC kernel, homography warp, the guards of
vq_flow_warped) and the helpers those tests share.  tests/test_warp_edges_oracle.py shows on the CPU that every input has the
property its GPU case relies on; tests/test_warp_edges_gpu.py runs them on the device.

Frames are uint8 [h, w].  Beside the textures of the older tests they make what a 256-thread block of corner_strength_kernel never
saw: pixel counts that are no multiple of 256 (dead lanes in the last block), the strongest response next to the border (reflect-101
applied twice), exact ties, a maximum that comes from the last partial block, a strong frame beside a weak one in one batch.  Match
sets are (src, dst) float32 [n, 2]."""
import functools

import numpy as np

import warp_oracle as wo
from test_warp_oracle import analytic_pair, synthetic_matches

F = np.float32
BLOCK = 256                                                   # threads of a block of the corner kernels (csrc/vq_flow.hip)
SMALL_SIZES = [(16, 16), (17, 19), (37, 53), (16, 300), (300, 16)]
FULL_SIZE = (256, 340)

# (max_corners, quality, min_distance): every value the issue lists, on every frame
CORNER_PARAMS = [(1000, 0.001, 0.0), (1000, 0.001, 0.5), (1000, 0.001, 1.0), (1000, 0.001, 2.5), (1000, 0.001, 4.5), (1000, 0.001, 10.0),
                 (25, 0.001, 2.5), (25, 0.5, 1.0), (25, 0.999, 10.0), (1, 0.001, 4.5), (1, 0.5, 0.0), (1000, 0.5, 0.5), (1000, 0.999, 2.5)]


# ---- frames --------------------------------------------------------------------------------------------------------------------

def uniform_noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def binary_noise(h, w, seed=0):
    """0 / 255 only: the largest gradients there are, many exactly equal strengths."""
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def low_contrast(img, base=126, levels=3):
    """The same texture squeezed into [base, base + levels]: its strengths shrink by (levels / 255)^2."""
    return (base + np.rint(img.astype(np.float64) * (levels / 255.0))).astype(np.uint8)


def _border_cells(n, cell, rim):
    """Cell index along one axis: a cell of `rim` pixels at 0, cells of `cell` pixels after it, a cell of `rim` pixels at the end."""
    i = np.arange(n)
    c = 1 + (i - rim) // cell
    c[:rim] = 0
    c[n - rim:] = c[n - rim - 1] + 1
    return c


def border_checker(h, w, cell=5, rim=2):
    """A 0 / 255 checkerboard free of noise whose outermost cells are `rim` pixels wide.  rim = 2: the outermost junctions lie between
    rows / columns 1 | 2 and n - 3 | n - 2, so rows / columns 1 and n - 2 carry peaks whose blocks read the reflected border; every cell
    edge runs out through rows / columns 0 and n - 1.  rim = 1: an edge between rows / columns 0 | 1, which reflect-101 turns into a line."""
    cy, cx = _border_cells(h, cell, rim), _border_cells(w, cell, rim)
    return (((cy[:, None] + cx[None, :]) % 2) * 255).astype(np.uint8)


def tail_start(h, w):
    """First pixel of the last block of a frame (the block with dead lanes when h * w is no multiple of 256)."""
    return ((h * w - 1) // BLOCK) * BLOCK


def tail_only(h, w, seed=0):
    """Flat except inside the last block of the frame."""
    img = np.full(h * w, 90, np.uint8)
    s = tail_start(h, w)
    img[s:] = np.random.default_rng(seed).integers(0, 256, h * w - s, dtype=np.uint8)
    return img.reshape(h, w)


def flat(h, w, value=77):
    return np.full((h, w), value, np.uint8)


def bright_pixel(h, w, last=False):
    img = np.zeros((h, w), np.uint8)
    img[(h - 1, w - 1) if last else (0, 0)] = 255
    return img


TAIL_SEEDS = {(16, 16): 0, (17, 19): 0, (37, 53): 0, (16, 300): 0, (300, 16): 0}


def small_frames(h, w):
    """name -> frame: every input family at one small size."""
    return {"noise": uniform_noise(h, w, seed=h + w), "binary": binary_noise(h, w, seed=h * w), "checker": border_checker(h, w), "rim checker": border_checker(h, w, rim=1),
            "tail": tail_only(h, w, seed=TAIL_SEEDS[(h, w)]), "flat": flat(h, w), "first pixel": bright_pixel(h, w),
            "last pixel": bright_pixel(h, w, last=True)}


def full_frame():
    """The textured 256 x 340 frame: more than 1000 corners at the default parameters."""
    return analytic_pair(FULL_SIZE[0], FULL_SIZE[1], np.eye(3), seed=31)[0]


def leak_batch(h=37, w=53):
    """[strong, weak, noise, strong]: binary noise, the same texture in four grey levels, uniform noise, the first frame again."""
    strong = binary_noise(h, w, seed=5)
    return np.stack([strong, low_contrast(strong), uniform_noise(h, w, seed=6), strong])


# ---- the corner oracle, each frame's maps computed once ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _maps(key, shape):
    img = np.frombuffer(key, np.uint8).reshape(shape)
    s = wo.corner_strength(img)
    return s, wo.corner_peaks(s)


def strength_and_peaks(img):
    img = np.ascontiguousarray(img, np.uint8)
    return _maps(img.tobytes(), img.shape)


@functools.lru_cache(maxsize=None)
def _corners(key, shape, cap, q, md):
    img = np.frombuffer(key, np.uint8).reshape(shape)
    s, peaks = _maps(key, shape)
    keep = (wo.corner_strength, wo.corner_peaks)
    wo.corner_strength, wo.corner_peaks = (lambda _img: s), (lambda _s: peaks)     # pure functions of the frame: computed once per frame
    try:
        out = wo.good_features(img, cap, q, md)
    finally:
        wo.corner_strength, wo.corner_peaks = keep
    out.setflags(write=False)
    return out


def oracle_corners(img, cap=wo.MAX_CORNERS, q=wo.QUALITY, md=wo.MIN_DISTANCE):
    """wo.good_features(img, cap, q, md), remembered: the GPU module and its CPU twin ask for the same lists."""
    img = np.ascontiguousarray(img, np.uint8)
    return _corners(img.tobytes(), img.shape, int(cap), float(q), float(md))


def corners_with_top(img, top, cap=wo.MAX_CORNERS, q=wo.QUALITY, md=wo.MIN_DISTANCE):
    """The corner list a frame would get if ANOTHER maximum were used for its quality threshold (what a leak between frames does)."""
    s, peaks = strength_and_peaks(img)
    forged = s.copy()
    forged[0, 0] = top                                        # row 0 is never a peak: only the maximum changes
    keep = (wo.corner_strength, wo.corner_peaks)
    wo.corner_strength, wo.corner_peaks = (lambda _img: forged), (lambda _s: peaks)
    try:
        return wo.good_features(img, cap, q, md)
    finally:
        wo.corner_strength, wo.corner_peaks = keep


# ---- match sets ----------------------------------------------------------------------------------------------------------------

H_PERSPECTIVE = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [2e-5, -1e-5, 1.0]])
THRESHOLD = 1.0


def _f(a):
    return np.ascontiguousarray(a, dtype=F).reshape(-1, 2)


def no_winner_sets():
    """name -> (src, dst): nothing valid can be drawn; the answer is winner -1, identity, 0 inliers, a zero mask."""
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(0, 340, 60), rng.uniform(0, 256, 60)], 1)
    k = np.arange(40)
    line = np.stack([k, 2 * k + 3], 1)                                      # whole numbers: every orientation is exactly 0
    two = np.tile(np.array([[31.5, 40.25], [200.0, 17.5]]), (30, 1))
    sets = {"n=0": (pts[:0], pts[:0]), "n=1": (pts[:1], pts[:1] + 1.0), "n=3": (pts[:3], pts[:3] + 1.0),
            "collinear": (line, line + np.array([3, -2])), "mirrored": (pts, np.stack([340.0 - pts[:, 0], pts[:, 1]], 1)),
            "two points": (two, two + np.array([2.0, -1.0]))}
    return {k: (_f(s), _f(d)) for k, (s, d) in sets.items()}


def small_sets():
    four = np.array([[10.0, 12.0], [200.0, 20.0], [190.0, 170.0], [15.0, 160.0]])
    five = np.vstack([four, [[100.0, 90.0]]])
    t = np.array([2.0, -1.0])
    return {"n=4": (_f(four), _f(four + t)), "n=5": (_f(five), _f(five + t))}


@functools.lru_cache(maxsize=None)
def full_set():
    """8192 matches: 6000 exact inliers of a perspective matrix, 2192 outliers displaced by 5 to 40 px."""
    s, d, inl = synthetic_matches(H_PERSPECTIVE, 6000, 2192, seed=41)
    return s, d, inl


@functools.lru_cache(maxsize=None)
def stride_set():
    """310 matches, 220 of them exact inliers: what the hypothesis counts around the 256 threads of the workgroup run on."""
    return synthetic_matches(H_PERSPECTIVE, 220, 90, seed=5)[:2]


STRIDE_HYPOTHESES = [1, 2, 255, 256, 257, 1000]
STRIDE_SEED = 11
# seeds for 1 and 2 hypotheses: under the first of each pair the oracle rejects every sample (winner -1), under the second its winner is 0
FEW_SEEDS = {1: (1, 0), 2: (54, 0)}


def batch_sets():
    """11 sets with different counts: one empty in the middle, one with 3 matches, two that have no winner."""
    A = np.array([[0.98, -0.03, -4.0], [0.03, 0.98, 6.0], [0, 0, 1.0]])
    nw = no_winner_sets()
    sets = [synthetic_matches(H_PERSPECTIVE, 120, 40, seed=50)[:2], synthetic_matches(A, 60, 25, seed=51)[:2], small_sets()["n=5"],
            synthetic_matches(np.eye(3), 30, 9, seed=52)[:2], nw["n=0"], synthetic_matches(A, 200, 100, seed=53)[:2], nw["n=3"],
            synthetic_matches(H_PERSPECTIVE, 17, 4, seed=54)[:2], nw["collinear"], small_sets()["n=4"], synthetic_matches(A, 90, 1, seed=55)[:2]]
    assert len({len(s) for s, _ in sets}) == len(sets)
    return sets


BATCH_ORDER = [7, 4, 0, 10, 2, 9, 8, 1, 6, 5, 3]          # the same sets in another order: each hashes with its new index


def pack(sets, max_points, pad=np.nan):
    """-> src, dst [n, max_points, 2] float32 filled with `pad` beyond each set's count, counts [n] int32."""
    src = np.full((len(sets), max_points, 2), pad, F)
    dst = np.full((len(sets), max_points, 2), pad, F)
    counts = np.array([len(s) for s, _ in sets], np.int32)
    for i, (s, d) in enumerate(sets):
        src[i, :len(s)], dst[i, :len(d)] = s, d
    return src, dst, counts


def ransac_margins(src, dst, threshold, hypotheses, seed, pair):
    """Every hypothesis of wo.ransac_homography evaluated once more, to judge how safe an equality test on its answer is.
    -> dict(winner, count, ties: hypotheses that reach the winning count, margin: the smallest |error^2 - threshold^2| of any match
    under ANY valid hypothesis, clear: the winner's count exceeds that of every hypothesis with another inlier set)."""
    n = len(src)
    thr2 = float(F(threshold)) ** 2
    found = []
    margin = np.inf
    if n >= 4:
        for j in range(hypotheses):
            idx = wo.draw_sample(seed, pair, j, n)
            if idx is None:
                continue
            s4, d4 = src[idx], dst[idx]
            if not all(wo._orient(s4[a], s4[(a + 1) & 3], s4[(a + 2) & 3]) * wo._orient(d4[a], d4[(a + 1) & 3], d4[(a + 2) & 3]) > 0 for a in range(4)):
                continue
            H = wo.homography_4pt(s4, d4)
            if H is None:
                continue
            e = wo.reprojection_error2(H, src, dst)
            margin = min(margin, float(np.abs(e - thr2).min()))
            found.append((j, e <= thr2))
    if not found:
        return {"winner": -1, "count": 0, "ties": 0, "margin": np.inf, "clear": True, "valid": 0}
    best = max(int(m.sum()) for _, m in found)
    winner, wmask = next((j, m) for j, m in found if int(m.sum()) == best)
    ties = sum(1 for _, m in found if int(m.sum()) == best)
    clear = all(int(m.sum()) < best or (m == wmask).all() for _, m in found)
    return {"winner": winner, "count": best, "ties": ties, "margin": margin, "clear": clear, "valid": len(found)}


# ---- homography warp -----------------------------------------------------------------------------------------------------------

WARP_SIZES = [(37, 53), (64, 80)]
FIXED_KW = dict(epsilon=0.0, iterations=20, warps=3, nscales=3)        # tests/test_flow_gpu.py: the fixed-count comparison, bound 1e-4 px
FIELD_BOUND = 1e-4


def translations(w):
    """(tx, ty) in pairs: the two of a pair ride in one batch with different matrices.  The last is wider than the frame."""
    return [((1, 0), (0, -1)), ((-1, 0), (0, 1)), ((5, -3), (w + 7, 0))]


def translation_matrix(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def shift_replicated(img, tx, ty):
    """out[y, x] = img[clamp(y - ty), clamp(x - tx)]: what a warp by the translation (tx, ty) shows, border replicated."""
    h, w = img.shape
    ys = np.clip(np.arange(h) - ty, 0, h - 1)
    xs = np.clip(np.arange(w) - tx, 0, w - 1)
    return np.ascontiguousarray(img[ys[:, None], xs[None, :]])


def warp_pair(h, w, seed=0):
    """A textured pair with a small motion of its own."""
    return analytic_pair(h, w, translation_matrix(1.5, -0.75), seed=seed)


# ---- vq_flow_warped: the batch of four ---------------------------------------------------------------------------------------------

GUARD_SIZE = (100, 141)
H_MILD = np.array([[1.002, 0.004, 2.5], [-0.003, 0.999, -1.5], [0.0, 0.0, 1.0]])


def blob_pair(h=GUARD_SIZE[0], w=GUARD_SIZE[1], rows=5, cols=10, move=2):
    """A flat frame carrying rows x cols isolated blobs (one corner each), all moved by `move` pixels to the right."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for dx in (0, move):
        img = np.full((h, w), 40.0)
        for r in range(rows):
            for c in range(cols):
                y0, x0 = 10 + r * (h - 20) / (rows - 1), 8 + c * (w - 20) / (cols - 1) + dx
                img += 180.0 * np.exp(-(((ys - np.rint(y0)) ** 2 + (xs - np.rint(x0)) ** 2) / (2 * 1.6 ** 2)))
        out.append(np.rint(img.clip(0, 255)).astype(np.uint8))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def guard_pairs():
    """name -> (frame0, frame1) at 100 x 141: (a) camera motion, (b) constant, (c) at most 50 corners, (d) unrelated textures."""
    h, w = GUARD_SIZE
    d0 = analytic_pair(h, w, np.eye(3), seed=61)[0]
    d1 = analytic_pair(h, w, np.eye(3), seed=62)[0]
    return {"a": analytic_pair(h, w, H_MILD, seed=60), "b": (flat(h, w, 128), flat(h, w, 128)), "c": blob_pair(), "d": (d0, d1)}


def guard_batch(order="abcd"):
    p = guard_pairs()
    return np.stack([p[k][0] for k in order]), np.stack([p[k][1] for k in order])
