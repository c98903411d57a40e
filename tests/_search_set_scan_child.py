"""Test program (GPU box): the one-query scan over a row view with ONE instantiation of scan_kernel forced.  ``VQ_SCAN_LEAN`` is read
once per process, so tests/test_search_set_gpu.py starts this file with 0 (streaming: the query slice lives in registers across clips)
and with 1 (lean), for float32 and float16 rows.

9 000 clips x 2 x 3, a seeded random view of ~7 000 rows: the grid is capped at 3 072 waves, so every wave walks two or three positions
-- the row index read ahead of the prefetch and the guard behind the wave's last clip.  Position i of the view scan must equal row
rows[i] of the same handle's full scan bit for bit; sampled rows are checked against the host regeneration (<= 1e-12).  Prints ``ok``."""
import os
import sys

lean, dtype_name = sys.argv[1], sys.argv[2]
os.environ["VQ_SCAN_LEAN"] = lean
os.environ.setdefault("VQ_NO_TORCH", "1")

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import sim_oracle as so
import video_query_algorithms_amd as vqa
from _search_set_cases import same_bits, same_values


def main():
    n, s, e, d, scales = 9000, 2, 3, 1024, (4.0, 1.0)
    dtype = {"f32": np.float32, "f16": np.float16}[dtype_name]
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=31, scales=scales, dtype=dtype)
    rng = np.random.default_rng(31)
    t = rng.standard_normal((s, e, d)) / d
    rows = np.flatnonzero(rng.random(n) < 7000 / n)
    assert 6800 <= rows.size <= 7200 and rows.size > 2 * 3072
    db.set_query(t)
    db.scan(weights=[1.0, 1.5], keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    sc = db.scores()
    db.define_search_rows("v", rows)
    db.use_search_set("v")
    db.scan(weights=[1.0, 1.5], keep_sims=True)
    v_avg, v_ne, v_sims = db.similarities(sims=True)
    v_sc = db.scores()
    assert v_avg.shape == (rows.size, s) and v_sims.shape == (rows.size, s, e)
    assert same_bits(v_avg, avg[rows]) and same_bits(v_ne, n_e[rows]) and same_bits(v_sims, sims[rows]) and same_bits(v_sc, sc[rows])
    assert same_values(v_sc, so.dense_scores(v_avg, [1.0, 1.5]))
    for lo in (0, rows.size // 2, rows.size - 48):
        part = rows[lo:lo + 48]
        x = np.concatenate([so.synth_features(31, int(r), 1, s, e, d, scales) for r in part]).astype(dtype)
        o_sims, o_avg, _ = so.dense_similarities(x.astype(np.float64), t)
        err = max(np.abs(v_sims[lo:lo + 48] - o_sims).max(), np.abs(v_avg[lo:lo + 48] - o_avg).max())
        print("lean=%s %s positions %d..: |d| = %.3g" % (lean, dtype_name, lo, err), flush=True)
        assert err <= 1e-12, (lo, err)
    db.close()


if __name__ == "__main__":
    main()
    print("ok", flush=True)
