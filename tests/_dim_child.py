"""Test program (GPU box): a database of logical length d padded by the LIBRARY (FeatureDB.from_arrays on rows of length d: vq_db_create
with the flags of include/vq_amd_dim.h, unpadded rows through vq_db_upload) against the same data zero-padded by numpy in a plain
database of D = d rounded up to a multiple of 4 (vq_db_create without flags).  ``VQ_SCAN_SHORT``
is read once per process, so tests/test_dim_gpu.py starts this file with 0: both handles then run scan_generic_kernel on the same
bytes, and everything they return must be EQUAL -- similarities, n_e, scores, the one-call round's lists, top-k, selection, lowest
score, loss surface, bootstrapped target (cut to d) and the rows read back.

    python tests/_dim_child.py <dtype>       # float32 | float64 | float16

d in {1, 3, 5, 101, 127, 129, 257} x (S, E) in {(1, 1), (2, 3)} x N in {1, 17, 130}, a presence mask, under a search set.  Prints ``ok``."""
import os
import sys

os.environ["VQ_SCAN_SHORT"] = "0"

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import video_query_algorithms_amd as vqa
from _dim_cases import draw, padded, same


def one(dtype, n, s, e, d, seed):
    rng = np.random.default_rng(seed)
    pitch = (d + 3) // 4 * 4
    x, present, rows, t = draw(rng, n, s, e, d, dtype)
    lib = vqa.FeatureDB.from_arrays(x, present=present, dtype=dtype)
    hand = vqa.FeatureDB(n, s, e, pitch, dtype, short_rows=False)
    hand.upload(0, padded(x, pitch))
    hand.set_present(present)
    assert (lib.D, lib.Dp, hand.D, hand.Dp) == (d, pitch, pitch, pitch)
    tag = (np.dtype(dtype).name, n, s, e, d)
    assert same(lib.read_rows(np.arange(n)), x) and same(hand.read_rows(np.arange(n))[..., :d], x), tag
    w = [1.0, 1.5][:s]
    th, lower = 0.7, 0.5
    m = rows.size
    for db in (lib, hand):
        db.define_search_rows("set", rows)
        db.use_search_set("set")
    lib.set_query(t)
    hand.set_query(padded(t, pitch))
    out = []
    for db in (lib, hand):
        db.scan(weights=w, keep_sims=True)
        avg, n_e, sims = db.similarities(sims=True)
        pos = np.arange(min(m, 3))
        wg = np.stack([np.ones(5), np.linspace(0.5, 2.5, 5)], axis=1)[:, :s]
        got = [avg, n_e, sims, db.scores(), *db.topk(min(5, m)), *db.select(th, lower), db.min_score(pos),
               db.loss_surface(wg, pos, (pos % 2).astype(np.float64), np.linspace(0.4, 0.9, 4), 0.1)]
        assert avg.shape == (m, s)
        out.append(got)
    for a, b in zip(*out):
        assert same(np.asarray(a), np.asarray(b)), tag
    tp = padded(t, pitch)
    ra, rb = lib.query_round(t, weights=w, select=(th, lower)), hand.query_round(tp, weights=w, select=(th, lower))
    for name in ("avg", "n_e", "scores", "match_rows", "near_rows"):
        assert same(getattr(ra, name), getattr(rb, name)), (tag, name)
    assert ra.near_argmax == rb.near_argmax and same(ra.avg, out[0][0]) and same(ra.scores, out[0][3]), tag
    # a second round on the reused block under a query whose pads would show if they were not written again
    ra2 = lib.query_round(2.0 * t, weights=w)
    rb2 = hand.query_round(2.0 * tp, weights=w)
    assert same(ra2.avg, rb2.avg) and same(ra2.scores, rb2.scores), tag
    valid = np.arange(min(n, 3, d))                                           # the validated clips of a problem are independent: at most d
    invalid = np.arange(5, 7) if n > 7 and valid.size + 2 <= d else np.arange(0)
    ba = lib.bootstrap_target(valid, invalid, mu=0.3, set_query=False)
    bb = hand.bootstrap_target(valid, invalid, mu=0.3, set_query=False)
    assert ba.shape == (s, e, d) and same(ba, bb[..., :d]) and not bb[..., d:].any(), tag
    qa, qb = lib.set_query_from_row(int(rows[0])), hand.set_query_from_row(int(rows[0]))
    assert qa.shape == (s, e, d) and same(qa, qb[..., :d]) and not qb[..., d:].any(), tag
    lib.close()
    hand.close()


if __name__ == "__main__":
    dtype = {"float32": np.float32, "float64": np.float64, "float16": np.float16}[sys.argv[1]]
    k = 0
    for d in (1, 3, 5, 101, 127, 129, 257):
        for s, e in ((1, 1), (2, 3)):
            for n in (1, 17, 130):
                one(dtype, n, s, e, d, 1000 + k)
                k += 1
    print("%d cases" % k, flush=True)
    print("ok", flush=True)
