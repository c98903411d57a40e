"""The k best clips of each of 16 queries of one batched pass: ranked on the device (FeatureDB.batch_round_topk) against the scores
copied back and ranked on the host.

    python tools/batch_topk_bench.py [--n 10000 1000000] [--k 20 1000] [--repeats 21]

Seeded and synthetic; fails when there is no GPU.  One process, after warm-up, the routes ALTERNATING (a repeat = each route once), so
drift of the shared host hits all alike; the host clock runs around a whole route, whose last device call ends in its own
synchronise; the figures are medians over the repeats, with the minimum and the maximum as the spread.  A resident n x 2 x 5 x 1024
fp32 database (cfg 4), 16 queries (scaled rows of it), no averaged similarities copied back in either route:

    (a)   query_round_batch(want_scores=False) + one batch_round_topk
    (b)   query_round_batch with the scores copied back (16 n doubles) + np_topk per query on the host -- what there was before
    pass  query_round_batch(want_scores=False) alone;  pass_scores  the same with the scores copied back
    topk  batch_round_topk alone, on the snapshot of a pass

(a) and (b) give the same positions and the same bits (checked here on every repeat).  One JSON line per (n, k).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

Q = 16


def _stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def np_topk(scores, k):
    """descending, ties by ascending position, NaNs excluded (tests/_search_set_cases.py)"""
    v = np.asarray(scores)
    idx = np.flatnonzero(~np.isnan(v))
    order = idx[np.lexsort((idx, -v[idx]))][:k]
    return order.astype(np.int64), v[order]


def bench(vqa, n, ks, repeats, warmup=3):
    s, e, d = 2, 5, 1024
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=17, scales=(4.0, 1.0))
    rows = db.read_rows([(37 * q + 1) % n for q in range(Q)]).astype(np.float64)
    targets = rows / (rows ** 2).sum(axis=-1, keepdims=True)
    weights = np.stack([[1.0, 0.6 + 0.1 * q] for q in range(Q)])

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def device_route(k):
        db.query_round_batch(targets, weights, want_avg=False, want_scores=False)
        return db.batch_round_topk(k)

    def host_route(k):
        r = db.query_round_batch(targets, weights, want_avg=False)
        return [np_topk(v.scores, k) for v in r]
    out = []
    for k in ks:
        for _ in range(warmup):
            device_route(k), host_route(k)
        a, b, p0, p1, t, same = [], [], [], [], [], True
        for _ in range(repeats):
            ms, got = timed(lambda: device_route(k))
            a.append(ms)
            got = [(np.array(r), np.array(v)) for r, v in got]
            ms, want = timed(lambda: host_route(k))
            b.append(ms)
            same = same and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1].view(np.int64), w[1].view(np.int64)) for g, w in zip(got, want))
            p1.append(timed(lambda: db.query_round_batch(targets, weights, want_avg=False))[0])
            p0.append(timed(lambda: db.query_round_batch(targets, weights, want_avg=False, want_scores=False))[0])
            t.append(timed(lambda: db.batch_round_topk(k))[0])
        sa, sb = _stats(a), _stats(b)
        out.append({"n": n, "S": s, "E": e, "D": d, "queries": Q, "k": k, "repeats": repeats, "form": "short" if n <= 16384 and k <= 1024 else "long",
                    "a_pass_and_device_topk_ms": sa, "b_pass_scores_back_and_host_topk_ms": sb, "pass_alone_ms": _stats(p0),
                    "pass_scores_back_ms": _stats(p1), "topk_alone_ms": _stats(t), "scores_back_bytes": Q * n * 8,
                    "a_faster_than_b": bool(sa["median"] < sb["median"]), "b_over_a": round(sb["median"] / sa["median"], 2),
                    "a_within_spread_of_b": bool(sa["median"] <= sb["median"] + (sb["max"] - sb["min"])), "same_rows_and_bits": bool(same)})
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 1_000_000], help="clips")
    ap.add_argument("--k", type=int, nargs="+", default=[20, 1000])
    ap.add_argument("--repeats", type=int, default=21)
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("at least 20 repeats")
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_topk_bench: no GPU -- nothing is measured without one")
    import video_query_algorithms_amd as vqa
    for n in args.n:
        for line in bench(vqa, n, args.k, args.repeats):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
