"""Test infrastructure: loss surfaces for the pick of a weight fit (Hyperparameter._pick_from / _pick_exact, the device's
pick_refine_batch_kernel) -- a seeded table of surfaces fitted from random labelled scores, crafted surfaces for every branch of the
pick, and a line-by-line restatement of the pick in plain loops.  Never imported by the product."""
import math
import os

import numpy as np

import sim_oracle as so

TABLE_SEED, TABLE_SIZE = 20260, 2400
FIT_TOLERANCE = 1e-6


def make_hp(vqa):
    return vqa.Hyperparameter({"rgb": 1.0, "warped_optical_flow": 1.5})


def candidates(hp, S=2):
    cand = np.zeros((len(hp.weight_grid), S))
    cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
    return cand


def fitted_surfaces(vqa, count=TABLE_SIZE, seed=TABLE_SEED):
    """[(raw surface [40][31], L)]: ``raw_loss_surface`` of L in 2 .. 60 clips with random averaged similarities, labelled by a noisy
    cut of their score under a random weight -- the surfaces a revise round meets, minima mostly inside the grid."""
    from video_query_algorithms_amd.hyperparameter import raw_loss_surface
    hp = make_hp(vqa)
    cand = candidates(hp)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        L = int(rng.integers(2, 61))
        avg = rng.random((L, 2)) ** 0.5
        w_true, th_true = rng.uniform(0.6, 2.3), rng.uniform(0.55, 1.0)
        truth = so.dense_scores(avg, [1.0, w_true]) + 0.04 * rng.standard_normal(L)
        labels = [bool(v) for v in truth >= np.quantile(truth, min(th_true, 0.95))]
        graded = np.stack([so.dense_scores(avg, w) for w in cand])
        out.append((raw_loss_surface(graded, labels, hp.threshold_grid, hp.ballast), L))
    return out


def bowl(G=40, T=31, at=(17, 12), steep=(0.013, 0.021)):
    """A smooth surface with its minimum at cell ``at``: separable parabolas over the cell indices."""
    g, t = np.meshgrid(np.arange(G, dtype=np.float64), np.arange(T, dtype=np.float64), indexing="ij")
    return 0.3 + steep[0] * (g - at[0]) ** 2 + steep[1] * (t - at[1]) ** 2


def crafted_surfaces():
    """name -> (raw surface [40][31], L): every branch of the pick."""
    G, T = 40, 31
    out = {}
    for name, at in (("rim-north", (17, T - 1)), ("rim-south", (17, 0)), ("rim-west", (0, 12)), ("rim-east", (G - 1, 12)),
                     ("corner", (G - 1, T - 1)), ("corner-00", (0, 0))):
        out[name] = (bowl(at=at), 7)
    out["interior"] = (bowl(at=(17, 12)) + 1e-4 * bowl(at=(19, 9)), 3)
    s = bowl(at=(9, 20))
    s[30, 5] = s[9, 20]
    out["tie-first-wins"] = (s, 5)
    s = bowl(at=(9, 20))
    s[3, 28] = s[9, 20]
    out["tie-earlier-row-wins"] = (s, 5)
    # 7 / 3 and 7.000000000000001 / 3 are one double apart as raw sums and the same double after the division by L = 3
    a, b = 7.0, float(np.nextafter(7.0, 8.0))
    assert a != b and a / 3 == b / 3
    s = 3 * bowl(at=(9, 20)) + 10.0
    s[20, 10], s[12, 4] = b, a
    out["tie-made-by-the-division"] = (s, 3)
    s = bowl(at=(9, 20))
    s[22, 7] = s[30, 1] = np.nan
    out["nan-first-nan-wins"] = (s, 4)
    s = bowl(at=(9, 20))
    s[9, 21] = np.nan
    out["nan-neighbour"] = (s, 4)
    s = bowl(at=(9, 20))
    s[:5] = np.inf
    s[9, 19] = np.inf
    out["inf-cells"] = (s, 4)
    out["all-inf"] = (np.full((G, T), np.inf), 4)
    out["all-equal"] = (np.full((G, T), 0.25 * 6), 6)
    s = np.full((G, T), 1e300)
    s[14, 14] = 9e299
    out["cells-of-1e300"] = (s, 2)
    s = bowl(at=(9, 20)) * 1e300
    out["overflowing-refinement"] = (s, 2)
    s = bowl(at=(9, 20))
    s[10, 20] = s[9, 20]
    out["tie-with-east"] = (s, 5)
    s = bowl(at=(9, 20))
    s[9, 21] = s[9, 20]
    out["tie-with-north"] = (s, 5)
    s = bowl(at=(9, 20))
    s[10, 20] = s[8, 20] = s[9, 21] = s[9, 19] = s[9, 20]
    out["flat-cross"] = (s, 5)
    s = -bowl(at=(9, 20))
    s[0, 0] = s[0, 1] = -0.0
    out["negative-surface"] = (s, 5)
    return out


def restated_pick(w_grid, th_grid, raw, L, eps):
    """hyperparameter.py:66-114 on raw / L, restated line by line over Python lists: (w_best, threshold, iw, it, on_rim, fell_back).
    Squares are products; a division by zero gives what IEEE gives (numpy scalars do, Python floats raise)."""
    G, T = len(w_grid), len(th_grid)
    cells = [[float(np.float64(raw[g][t]) / np.float64(L)) for t in range(T)] for g in range(G)]
    iw = it = None
    for g in range(G):                                         # numpy.argmin: the first NaN, else the first smallest
        for t in range(T):
            v = cells[g][t]
            if iw is None:
                iw, it = g, t
            elif not math.isnan(cells[iw][it]) and (math.isnan(v) or v < cells[iw][it]):
                iw, it = g, t
    on_rim = iw in (0, G - 1) or it in (0, T - 1)
    if on_rim:
        return float(w_grid[iw]), float(th_grid[it]) - eps, iw, it, True, False

    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    def parabola(lo, mid, hi, y_lo, y_mid, y_hi):
        rise, fall_hi, fall_lo = y_hi - y_lo, y_mid - y_hi, y_mid - y_lo
        vertex = div(0.5 * (rise * (mid * mid) + fall_hi * (lo * lo) - fall_lo * (hi * hi)), rise * mid + fall_hi * lo - fall_lo * hi)
        return vertex, div(fall_lo, (mid - vertex) * (mid - vertex) - (lo - vertex) * (lo - vertex))
    ws = [float(w_grid[iw - 1]), float(w_grid[iw]), float(w_grid[iw + 1])]
    ths = [float(th_grid[it - 1]), float(th_grid[it]), float(th_grid[it + 1])]
    centre, west, east, south, north = cells[iw][it], cells[iw - 1][it], cells[iw + 1][it], cells[iw][it - 1], cells[iw][it + 1]
    w0, a = parabola(ws[0], ws[1], ws[2], west, centre, east)
    th0, b = parabola(ths[0], ths[1], ths[2], south, centre, north)
    c = centre - a * ((ws[1] - w0) * (ws[1] - w0)) - b * ((ths[1] - th0) * (ths[1] - th0))
    w0 = ws[2] if ws[2] < w0 else w0                           # min(w0, ws[2])
    w0 = ws[0] if ws[0] > w0 else w0                           # max(., ws[0])
    th0 = ths[2] if ths[2] < th0 else th0
    th0 = ths[0] if ths[0] > th0 else th0

    def model(w, t):
        return a * ((w - w0) * (w - w0)) + b * ((t - th0) * (t - th0)) + c
    misfit = (abs(west - model(ws[0], ths[1])) + abs(south - model(ws[1], ths[0])) + abs(centre - model(ws[1], ths[1]))
              + abs(north - model(ws[1], ths[2])) + abs(east - model(ws[2], ths[1])))
    if misfit > FIT_TOLERANCE:
        return ws[1], ths[1] - eps, iw, it, False, True
    return w0, th0 - eps, iw, it, False, False


def exact_pick(hp, raw, L):
    """(w_best, threshold, iw, it, on_rim, fell_back) of ``Hyperparameter._pick_exact`` on raw / L, as plain floats."""
    with np.errstate(all="ignore"):
        weights, th, iw, it, on_rim, fell_back = hp._pick_exact(np.asarray(raw) / L)
    return float(weights[hp.streams[1]]), float(th), iw, it, on_rim, fell_back


def same_pick(a, b):
    """Two picks agree bit for bit (a NaN weight or threshold equals a NaN one)."""
    return np.array_equal(np.array(a[:2]), np.array(b[:2]), equal_nan=True) and tuple(a[2:]) == tuple(b[2:])


def compute_eps():
    return float(os.environ["COMPUTE_EPS"])
