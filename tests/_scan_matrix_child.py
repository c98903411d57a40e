"""Test program (GPU box): EVERY (S, E) entry of the one-query dispatch at D = 1024 for one storage type, with ONE instantiation of
scan_kernel forced.  ``VQ_SCAN_LEAN`` is read once per process, so tests/test_scan_matrix_gpu.py starts this file with 0 (streaming: the
query slice lives in registers across clips) and with 1 (lean), for float16, float32 and float64 rows; ``cus`` is the device's
number of compute units (the parent has torch).  Per shape:

  * exact rows: 1 024 one-hot clips (_scan_matrix_cases.one_hot_rows) -- the similarities equal the oracle's EXACTLY;
  * looping waves: n = 2 W + 3 clips for the W waves the launch rule gives the shape, so every wave walks two clips and three walk a
    third: rows sampled from the head, the middle and the end against the host regeneration (<= 1e-12), scores bit for bit,
    a second scan the same bits; then a random view of ~70 % of the rows (more than W: view waves loop too), bit for bit the full scan;
  * for one shape per S the same under a presence mask with (clip, stream) pairs that have no split present: NaN there, nowhere else.

Prints one line per shape and ``ok``."""
import os
import sys

lean, dtype_name, cus = sys.argv[1], sys.argv[2], int(sys.argv[3])
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
from _scan_matrix_cases import D, DTYPES, MASKED, SCALES, SHAPES, WEIGHTS, check_sampled, one_hot_rows, sample_positions, shape_line, waves
from _search_set_cases import presence_mask, same_bits, same_values

dtype = DTYPES[dtype_name]


def exact_rows(s, e):
    n = 1024
    x, t = one_hot_rows(n, s, e, dtype)
    k = np.argmax(x != 0, axis=3)                                                      # [n, s, e]: where each vector's non-zero is
    assert ((x != 0).sum(axis=3) == 1).all() and all(np.unique(k[:, v // e, v % e]).size == D for v in range(s * e))
    db = vqa.FeatureDB.from_arrays(x, dtype=dtype)
    db.set_query(t)
    db.scan(keep_sims=True)
    _, _, sims = db.similarities(sims=True)
    o_sims, _, _ = so.dense_similarities(x.astype(np.float64), t)
    assert (sims == o_sims).all(), ("one-hot rows", s, e, int((sims != o_sims).sum()))
    # more than 1 024 distinct values; at 1 x 1 there are only 1 024 similarities (products of 7 values and 1 024): more than half
    assert len(np.unique(sims)) > (1024 if s * e > 1 else 512)
    db.close()


def scan(db, w):
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    return avg, n_e, sims, db.scores()


def under_view(db, w, rows, full):
    db.define_search_rows("v", rows)
    db.use_search_set("v")
    got = scan(db, w)
    assert got[0].shape == (rows.size, db.S) and got[2].shape == (rows.size, db.S, db.E)
    assert all(same_bits(a, b[rows]) for a, b in zip(got, full)), "view"
    db.use_search_set(None)
    db.drop_search_set("v")


def looping_waves(s, e):
    W = waves(cus, s, e)
    n = 2 * W + 3
    assert n > 2 * W
    seed, w = 100 + 10 * s + e, WEIGHTS[:s]
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s], dtype=dtype)
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((s, e, D)) / D
    rows = np.flatnonzero(rng.random(n) < 0.7)
    assert W < rows.size < n
    db.set_query(t)
    full = scan(db, w)
    avg, n_e, sims, sc = full
    assert (n_e == e).all()
    at = sample_positions(n)
    err = check_sampled(seed, s, e, dtype, t, at, sims[at], avg[at], n_e[at])
    assert (sc == so.dense_scores(avg, w)).all()
    assert all(same_bits(a, b) for a, b in zip(scan(db, w), full)), "second scan"
    under_view(db, w, rows, full)
    at = sample_positions(rows.size)                           # the view's own head, middle and end
    check_sampled(seed, s, e, dtype, t, rows[at], sims[rows[at]], avg[rows[at]], n_e[rows[at]])
    masked = ""
    if MASKED[s] == (s, e):
        present = presence_mask(n, s, e)
        assert (present[1, 0] == 0).all() and (present[n - 1, s - 1] == 0).all()
        db.set_present(present)
        m_full = scan(db, w)
        avg, n_e, sims, sc = m_full
        assert (n_e == present.sum(axis=2)).all() and (np.isnan(avg) == (n_e == 0)).all()
        assert np.isnan(avg[1, 0]) and n_e[1, 0] == 0 and np.isnan(avg[n - 1, s - 1]) and n_e[n - 1, s - 1] == 0
        at = sample_positions(n)                               # rows 1 and n - 1 are among them
        check_sampled(seed, s, e, dtype, t, at, sims[at], avg[at], n_e[at], present)
        assert same_values(sc, so.dense_scores(avg, w)) and (np.isnan(sc) == (n_e == 0).any(axis=1)).all()
        assert all(same_bits(a, b) for a, b in zip(scan(db, w), m_full)), "second masked scan"
        under_view(db, w, rows, m_full)
        masked = " masked: %d (clip, stream) without a split" % int((n_e == 0).sum())
    db.close()
    return n, W, rows.size, err, masked


if __name__ == "__main__":
    for s, e in SHAPES:
        exact_rows(s, e)
        n, W, m, err, masked = looping_waves(s, e)
        print("%s lean=%s %s one-hot exact; n = %d on %d waves, view of %d, |d| = %.3g%s" % (shape_line(s, e), lean, dtype_name, n, W, m, err, masked),
              flush=True)
    print("ok", flush=True)
