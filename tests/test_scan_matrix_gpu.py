"""GPU: every compiled variant of the one-query similarity scans (csrc/vq_sim.hip) against oracle/sim_oracle.py.

launch_scan compiles scan_kernel for 3 storage types x 10 (S, E) shapes x lean / streaming x plain / row view and scan_tiled_kernel
for the 10 shapes x plain / row view.  Here every one of them is launched, with more clips (tiles) than the grid has waves, so that each
wave walks a second item and a few a third: the prefetch of the wave's next clip, the guard behind its last one and, under a view,
the row index fetched two items ahead only run then.

  * scan_kernel: tests/_scan_matrix_child.py, one fresh process per (lean, dtype) -- ``VQ_SCAN_LEAN`` is read once per process;
  * scan_tiled_kernel: below, in this process (fp32 is the only tiled storage type)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sim_oracle as so
from _scan_matrix_cases import D, SCALES, SHAPES, TOL, WEIGHTS, check_sampled, sample_positions, shape_line, tile_view_rows, waves
from _search_set_cases import same_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


@pytest.fixture(scope="module")
def cus(gpu):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("lean", ["0", "1"])
@pytest.mark.parametrize("dtype", ["f16", "f32", "f64"])
def test_every_shape_of_the_scan_kernel_with_looping_waves(cus, lean, dtype):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_scan_matrix_child.py"), lean, dtype, str(cus)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
    lines = r.stdout.splitlines()
    for s, e in SHAPES:                                        # no entry of the table was skipped
        assert sum(line.startswith(shape_line(s, e)) for line in lines) == 1, (s, e, r.stdout[-4000:])


def _scan(db, w):
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    return avg, n_e, sims, db.scores()


@pytest.mark.parametrize("s,e", SHAPES)
def test_every_shape_of_the_tiled_scan_with_more_tiles_than_waves(vqa, cus, s, e):
    """n = 16 (2 W) + 5 clips: 2 W + 1 tiles on W waves, the last tile holds 5 clips.  The tiled handle against a row-major one of the
    same seed (n_e equal, avg and sims <= 1e-12) and both against the oracle on sampled rows; scores bit for bit from the tiled avg; a
    second scan the same bits; a view with untouched tiles and tiles touched in one clip == the tiled full scan at its rows, bit for bit."""
    W = waves(cus, s, e)
    n = 16 * (2 * W) + 5
    ntiles = (n + 15) // 16
    assert ntiles > 2 * W and n % 16 == 5
    seed, w = 200 + 10 * s + e, WEIGHTS[:s]
    t = np.random.default_rng(seed).standard_normal((s, e, D)) / D
    rows_db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s])
    rows_db.set_query(t)
    r_avg, r_ne, r_sims, r_sc = _scan(rows_db, w)
    rows_db.close()
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s])
    db.set_layout("tiled")
    assert db.layout == "tiled"
    db.set_query(t)
    full = _scan(db, w)
    avg, n_e, sims, sc = full
    assert (n_e == r_ne).all() and (n_e == e).all()
    assert np.abs(avg - r_avg).max() <= TOL and np.abs(sims - r_sims).max() <= TOL
    at = sample_positions(n)
    err_t = check_sampled(seed, s, e, np.float32, t, at, sims[at], avg[at], n_e[at])
    err_r = check_sampled(seed, s, e, np.float32, t, at, r_sims[at], r_avg[at], r_ne[at])
    assert (sc == so.dense_scores(avg, w)).all() and (r_sc == so.dense_scores(r_avg, w)).all()
    assert all(same_bits(a, b) for a, b in zip(_scan(db, w), full)), "second scan"
    rows = tile_view_rows(n, seed)
    touched = np.unique(rows >> 4).size
    assert W < touched < ntiles                                # view waves walk a second tile too
    db.define_search_rows("v", rows)
    db.use_search_set("v")
    got = _scan(db, w)
    assert got[0].shape == (rows.size, s) and got[2].shape == (rows.size, s, e)
    assert all(same_bits(a, b[rows]) for a, b in zip(got, full)), "view"
    print("%s tiled n = %d, %d tiles on %d waves, view of %d rows in %d tiles, |d| tiled %.3g rows %.3g" % (shape_line(s, e), n, ntiles, W, rows.size,
                                                                                                           touched, err_t, err_r))
    db.close()
