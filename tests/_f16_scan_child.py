"""Test program (GPU box): the one-query scan of a float16 database with ONE instantiation of scan_kernel forced.  ``VQ_SCAN_LEAN`` is
read once per process, so tests/test_f16_db_gpu.py starts this file once with 0 (streaming: the query slice lives in registers across
clips) and once with 1 (lean: re-read from LDS per clip).

  * every k position: 2 048 one-hot rows (row c, vector v: one non-zero at k = (7 c + 131 v) mod 1024) against a query of distinct
    values per k.  Each dot has ONE term and the product is exact, so the similarities must equal the oracle's exactly;
  * waves that loop: 40 003 clips x 2 x 3 (3 072 waves of 13 or 14 clips, a ragged last round), rows sampled from the head, the
    middle and the last 40 against the host regeneration rounded to float16, <= 1e-12.

Prints ``ok``."""
import os
import sys

lean = sys.argv[1]
os.environ["VQ_SCAN_LEAN"] = lean
os.environ.setdefault("VQ_NO_TORCH", "1")

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sim_oracle as so
import video_query_algorithms_amd as vqa
from _scan_matrix_cases import one_hot_rows


def one_hot():
    x, t = one_hot_rows(2048, 2, 3, np.float16)                                        # exact halves; distinct per (v, k); products are exact
    db = vqa.FeatureDB.from_arrays(x, dtype=np.float16)
    db.set_query(t)
    db.scan(keep_sims=True)
    _, _, sims = db.similarities(sims=True)
    o_sims, _, _ = so.dense_similarities(x.astype(np.float64), t)
    assert (sims == o_sims).all(), ("one-hot rows", int((sims != o_sims).sum()))
    assert len(np.unique(sims)) > 1024
    db.close()


def looping_waves():
    n, s, e, d, scales = 40_003, 2, 3, 1024, (4.0, 1.0)
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=29, scales=scales, dtype=np.float16)
    t = np.random.default_rng(29).standard_normal((s, e, d)) / d
    db.set_query(t)
    db.scan(weights=[1.0, 1.5], keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    sc = db.scores()
    assert (n_e == e).all()
    for row0, rows in ((0, 64), (n // 2 - 7, 64), (n - 40, 40)):
        x16 = so.synth_features(29, row0, rows, s, e, d, scales).astype(np.float16)
        o_sims, o_avg, _ = so.dense_similarities(x16.astype(np.float64), t)
        err = max(np.abs(sims[row0:row0 + rows] - o_sims).max(), np.abs(avg[row0:row0 + rows] - o_avg).max())
        print("lean=%s rows %d..%d: |d| = %.3g" % (lean, row0, row0 + rows, err), flush=True)
        assert err <= 1e-12, (row0, err)
    assert (sc == so.dense_scores(avg, [1.0, 1.5])).all()
    db.scan(weights=[1.0, 1.5], keep_sims=True)
    assert (db.similarities()[0] == avg).all() and (db.scores() == sc).all()          # bit-reproducible
    db.close()


if __name__ == "__main__":
    one_hot()
    looping_waves()
    print("ok", flush=True)
