"""Seeded frame pairs for the TV-L1 tests and the comparison helpers those tests share (tests/test_flow_edges_oracle.py checks the
helpers themselves on injected errors; tests/test_flow_edges_gpu.py uses them on the device's results).

Builders return (frame0, frame1), uint8 [h, w].  Beside the smooth, box-blurred texture of test_flow_oracle._shifted_pair they make
what that texture never shows the kernels: flat regions (|grad|^2 <= 1e-10: the fourth case of the thresholding step), hard edges,
saturation, whole-pixel motion of white noise, a brightness change without motion, motion that points out of the frame, occlusion.
``hard_pair`` puts several of them into one frame."""
import numpy as np

import tvl1_oracle as tv
from test_flow_oracle import _shifted_pair

F = np.float32


def shifted_pair(h, w, dx, dy, seed=0, margin=24):
    """The smooth texture of the existing tests, moved by (dx, dy)."""
    return _shifted_pair(h, w, dx, dy, seed=seed, margin=margin)


def _move(img, dx, dy, fill=0):
    """img moved by whole pixels (content at x goes to x + dx), the uncovered border filled with `fill`."""
    h, w = img.shape
    out = np.full_like(img, fill)
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[yd, xd] = img[ys, xs]
    return out


def square_on_black(h, w, seed=0):
    """A bright square that moves by whole pixels over flat black: |grad| = 0 and rho = 0 almost everywhere."""
    rng = np.random.default_rng(seed)
    side = max(3, min(h, w) // 3)
    y0, x0 = int(rng.integers(1, max(2, h - side - 2))), int(rng.integers(1, max(2, w - side - 2)))
    f0 = np.zeros((h, w), np.uint8)
    f0[y0:y0 + side, x0:x0 + side] = int(rng.integers(180, 256))
    return f0, _move(f0, int(rng.integers(1, 3)), int(rng.integers(-2, 1)))


def noise_band(h, w, seed=0):
    """A band of uniform white noise that moves by whole pixels between flat grey borders."""
    rng = np.random.default_rng(seed)
    f0 = np.full((h, w), 128, np.uint8)
    f0[h // 4:h - h // 4] = rng.integers(0, 256, (h - 2 * (h // 4), w), dtype=np.uint8)
    return f0, _move(f0, int(rng.integers(1, 4)), 0, fill=128)


def brightness_band(h, w, seed=0):
    """Flat everywhere; a band changes its brightness between the frames and nothing moves."""
    rng = np.random.default_rng(seed)
    f0 = np.full((h, w), 60, np.uint8)
    f1 = f0.copy()
    f0[h // 3:h - h // 3] = int(rng.integers(90, 110))
    f1[h // 3:h - h // 3] = int(rng.integers(130, 160))
    return f0, f1


def checkerboard(h, w, seed=0, cell=5):
    """Step edges between 0 / 255 free of any noise (exact ties everywhere), moved by one or two pixels."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    dx, dy = int(rng.integers(1, 3)), int(rng.integers(0, 2))
    f0 = ((((ys // cell) + (xs // cell)) % 2) * 255).astype(np.uint8)
    f1 = (((((ys - dy) // cell) + ((xs - dx) // cell)) % 2) * 255).astype(np.uint8)
    return f0, f1


def saturated(h, w, seed=0):
    """The smooth texture with its contrast tripled and clipped: large areas at exactly 0 and exactly 255, moving edges between."""
    rng = np.random.default_rng(seed)
    a, b = _shifted_pair(h, w, float(rng.uniform(-2.5, 2.5)), float(rng.uniform(-1.5, 1.5)), seed=seed)
    sat = lambda f: np.clip((f.astype(np.float64) - 127.5) * 3.0 + 127.5, 0, 255).round().astype(np.uint8)   # noqa: E731
    return sat(a), sat(b)


def leaving(h, w, seed=0):
    """A shift of 9 to 12 pixels: near the border the flow points out of the frame (the clamp of the bilinear sampler)."""
    rng = np.random.default_rng(seed)
    s = float(rng.uniform(9.0, 12.0)) * (1 if seed % 2 else -1)
    return _shifted_pair(h, w, s, float(rng.uniform(-1.0, 1.0)), seed=seed, margin=24)


def identical(h, w, seed=0):
    f0 = _shifted_pair(h, w, 0.0, 0.0, seed=seed)[0]
    return f0, f0.copy()


BUILDERS = {"square": square_on_black, "noise": noise_band, "brightness": brightness_band, "checker": checkerboard, "saturated": saturated,
            "leaving": leaving, "identical": identical}


def hard_pair(h, w, seed=0):
    """Five bands from top to bottom -- saturated texture | bright square on black beside a checkerboard | a flat band that changes its
    brightness | whole-pixel white noise | texture leaving the frame -- and on top of them a textured square that moves on its own and
    covers / uncovers what lies behind it (occlusion)."""
    rng = np.random.default_rng(1000 + seed)
    edges = [0, h // 4, h // 2, (5 * h) // 8, (3 * h) // 4, h]
    parts = [saturated(h, w, seed), None, brightness_band(h, w, seed), noise_band(h, w, seed), leaving(h, w, seed)]
    sq, ch = square_on_black(h, w, seed), checkerboard(h, w, seed)
    parts[1] = tuple(np.concatenate([s[:, :w // 2], c[:, w // 2:]], axis=1) for s, c in zip(sq, ch))
    out = []
    for k in range(2):
        f = np.empty((h, w), np.uint8)
        for b in range(5):
            rows = slice(edges[b], edges[b + 1])
            src = parts[b][k]
            if b == 1:          # the square of square_on_black sits anywhere: show the rows around it
                y0 = int(np.argmax(sq[0].any(axis=1)))
                top = min(max(0, y0 - 1), h - (edges[2] - edges[1]))
                f[rows] = src[top:top + edges[2] - edges[1]]
            elif b == 2:        # ... and the rows where the brightness changes
                f[rows] = src[h // 2]
            elif b == 3:
                f[rows] = src[h // 4:h // 4 + edges[4] - edges[3]]
            else:
                f[rows] = src[rows]
        out.append(f)
    side = max(3, min(h, w) // 4)
    tex = _shifted_pair(side, side, 0.0, 0.0, seed=seed + 77)[0]
    y0, x0 = int(rng.integers(0, h - side + 1)), int(rng.integers(0, w - side + 1))
    y1, x1 = min(max(y0 - 3, 0), h - side), min(max(x0 + 4, 0), w - side)
    out[0][y0:y0 + side, x0:x0 + side] = tex
    out[1][y1:y1 + side, x1:x1 + side] = tex
    return out[0], out[1]


def stack(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ---- comparison helpers ---------------------------------------------------------------------------------------------------------

FIELD_BOUND = 1e-4         # px: the project's bound for device against oracle when both run the same iterations (tests/test_flow_gpu.py)


def same_bits(a, b):
    """Two device results are the same bits (not merely equal: -0.0 and NaNs count)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def field_difference(got_u1, got_u2, want_u1, want_u2):
    """Largest absolute difference of the two fields in px (inf when a value is not finite)."""
    if not (np.isfinite(got_u1).all() and np.isfinite(got_u2).all() and np.isfinite(want_u1).all() and np.isfinite(want_u2).all()):
        return float("inf")
    return float(max(np.abs(got_u1.astype(np.float64) - want_u1).max(), np.abs(got_u2.astype(np.float64) - want_u2).max()))


def assert_fields_match(got_u1, got_u2, want_u1, want_u2, what="", bound=FIELD_BOUND):
    d = field_difference(got_u1, got_u2, want_u1, want_u2)
    assert d <= bound, "%s: fields differ by %.3g px (bound %.1g)" % (what, d, bound)
    return d


def audit_decisions(counts, trace, epsilon, cap, d):
    """Were the stop decisions behind `counts` right?  counts [level][warp] = the iterations a pair ran, trace [level][warp][iteration] =
    the oracle's fp64 mean squared updates on the SAME schedule.  Every iteration is one decision: before the last the error must be
    > eps^2 (go on), at the last <= eps^2 (stop) unless the last is the cap.  A decision is exempt as grazing only when
    |error / eps^2 - 1| < g = 4 d / epsilon, d = this pair's measured field difference against that oracle run: the update is a difference
    of two fields each off by at most d and its rms at the decision is about epsilon, so the sum changes by at most 4 d / epsilon of itself.
    -> (decisions, exempted); AssertionError on a wrong decision."""
    eps = float(F(epsilon))
    eps2 = eps * eps
    g = 4.0 * d / eps
    decisions = exempt = 0
    for lvl, (cl, tl) in enumerate(zip(counts, trace)):
        for wp, (k, errs) in enumerate(zip(cl, tl)):
            k = int(k)
            assert len(errs) == k and 1 <= k <= cap, "level %d warp %d: %d iterations, trace of %d, cap %d" % (lvl, wp, k, len(errs), cap)
            for i, e in enumerate(errs):
                decisions += 1
                right = (e > eps2) if i < k - 1 else (e <= eps2 or k == cap)
                if right:
                    continue
                assert abs(e / eps2 - 1.0) < g, ("level %d warp %d iteration %d of %d: error / eps^2 = %.9g is a wrong decision (grazing band %.3g)"
                                                % (lvl, wp, i + 1, k, e / eps2, g))
                exempt += 1
    return decisions, exempt


def case_counts(f0, f1, **kw):
    """Cells per case of the thresholding step (rho < -l_t g, rho > l_t g, in between with a gradient, in between without) over a whole
    oracle run of the pair: which branches an input reaches."""
    c = np.zeros(4, np.int64)
    tv.tvl1_flow(f0, f1, case_counts=c, **kw)
    return c
