"""Test infrastructure for the scan matrix (tests/test_scan_matrix_gpu.py, tests/_scan_matrix_child.py): every (S, E) entry of the
one-query dispatch in csrc/vq_sim.hip, the launch rule that says how many waves a scan gets, one-hot rows whose dots are exact in
every storage type, and the comparison of sampled rows with the host regeneration of a synthetic database."""
import numpy as np

import sim_oracle as so

D = 1024
SHAPES = [(s, e) for s in (1, 2) for e in (1, 2, 3, 4, 5)]     # the C_(s_, e_) table of launch_scan: a new entry gets a new row here
MASKED = {1: (1, 4), 2: (2, 5)}                                # per S, the shape that also runs under a presence mask
SCALES = (4.0, 1.0)
WEIGHTS = [1.0, 1.5]
TOL = 1e-12                                                    # the project's tolerance for a dot product (tests/test_sim_gpu.py)
DTYPES = {"f16": np.float16, "f32": np.float32, "f64": np.float64}


def shape_line(s, e):
    """What a child prints per shape and the parent looks for."""
    return "shape %d x %d:" % (s, e)


def waves(cus, s, e):
    """launch_scan_t: workgroups of 4 waves, as many per compute unit as fit its 160 KiB of LDS next to the fp64 query image
    (S E 8 KiB at D = 1024), 8 at the most.  A database of more clips (tiled: tiles) than this makes waves loop."""
    per_cu = max(1, min(8, (160 * 1024) // (s * e * D * 8)))
    return cus * per_cu * 4


def one_hot_rows(n, s, e, dtype):
    """(x [n,s,e,D], t [s,e,D]): row c, vector v has ONE non-zero, 1 + (c mod 7) / 4, at k = (7 c + 131 v) mod D; query element i is
    (1 + i) 2^-16.  A dot is one product of a 4-bit by a 14-bit significand: exact in float16, float32 and float64, whatever the
    order of the sum."""
    x = np.zeros((n, s, e, D), dtype=dtype)
    c = np.arange(n)
    for v in range(s * e):
        x[c, v // e, v % e, (7 * c + 131 * v) % D] = 1.0 + 0.25 * (c % 7)
    t = ((1.0 + np.arange(s * e * D)) * 2.0 ** -16).reshape(s, e, D)
    return x, t


def sample_positions(m):
    """64 from the head, 64 from the middle and the last 40 of m positions"""
    return np.concatenate([np.arange(0, 64), np.arange(m // 2 - 7, m // 2 + 57), np.arange(m - 40, m)])


def check_sampled(seed, s, e, dtype, t, rows, sims, avg, n_e, present=None):
    """Database rows ``rows`` of the synthetic database (seed, s, e), regenerated on the host, rounded to ``dtype`` and fed to the
    oracle, against what a scan returned for them: sims and avg <= 1e-12 (NaN exactly where the oracle has no split present), n_e
    equal.  Returns the largest difference."""
    x = np.concatenate([so.synth_features(seed, int(r), 1, s, e, D, SCALES[:s]) for r in rows]).astype(dtype)
    o_sims, o_avg, o_ne = so.dense_similarities(x.astype(np.float64), t, None if present is None else present[rows])
    assert (n_e == o_ne).all()
    assert (np.isnan(avg) == np.isnan(o_avg)).all() and (np.isnan(o_avg) == (o_ne == 0)).all() and not np.isnan(sims).any()
    fin = ~np.isnan(o_avg)
    err = max(np.abs(sims - o_sims).max(), np.abs(avg[fin] - o_avg[fin]).max())
    assert err <= TOL, err
    return err


def tile_view_rows(n, seed):
    """Rows of a view over a tiled database of n clips: per tile of 16, by turns one clip, all sixteen, or a random subset -- of
    those tiles every tenth is not touched at all; the ragged last tile whole."""
    ntiles = (n + 15) // 16
    tile = np.arange(ntiles)
    keep = np.random.default_rng(seed).random((ntiles, 16)) < 0.4
    keep[tile % 3 == 0] = False
    keep[tile % 3 == 0, 5] = True
    keep[tile % 3 == 1] = True
    keep[(tile % 3 == 2) & (tile % 10 == 0)] = False
    keep[ntiles - 1] = True
    rows = np.flatnonzero(keep.reshape(-1)[:n]).astype(np.int64)
    per_tile = np.bincount(rows >> 4, minlength=ntiles)
    assert (per_tile == 0).any() and (per_tile == 1).any() and (per_tile == 16).any() and rows[-1] == n - 1
    return rows
