"""Sixteen pending tickets on a row-sharded database: their own query rounds against one batched round.

    python tools/batch_sharded_bench.py [--n 10000] [--repeats 11] [--k 20]

Seeded and synthetic; fails when there is no GPU.  A served ShardedFeatureDB of world 2 over gloo, BOTH RANKS ON ONE CARD, on an
n x 2 x 3 x 1024 fp32 store: the figures show the calls and the bytes a batched round saves between the ranks, not multi-GPU scaling.
One broker process, after warm-up, the two routes ALTERNATING (a repeat = each route once), so drift of the shared host hits both
alike; the host clock runs around a whole route, whose last call ends in a gather that the host reads; medians over the repeats,
with the minimum and the maximum as the spread.

    (a)  16 x ShardedFeatureDB.query_round(t, weights, select): every ticket's own round -- what a sharded database did before
         batch_rounds=True, and still does without it
    (b)  one query_round_batch(want_avg=False, want_scores=False) with the 16 bands + one batch_round_topk(k)

Next to the times: the announcements, and the number and the sizes of the all-gathers of each route (counted in this process).
(b)'s pass runs on the matrix cores, so its scores agree with (a)'s to rounding (<= 1e-12), not bit for bit: the largest difference
between (b)'s ranked values and the k best of (a)'s scores is reported.  One JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

Q = 16


def _stats(v):
    v = sorted(v)
    return {"min": round(v[0], 3), "median": round(v[len(v) // 2], 3), "max": round(v[-1], 3)}


class _Traffic:
    """Counts the announcements and the all-gathers of sharded_db in this process: (rows of the result, bytes of the result)."""

    def __init__(self, sharded_db, cls):
        self.mod, self.cls, self.gathers, self.announced = sharded_db, cls, [], 0
        self.real = (sharded_db.all_gather_rows, sharded_db.all_gather_counts, cls._announce)
        outer = self

        def rows(local, n_total, group=None):
            outer.gathers.append((int(n_total), int(n_total) * int(np.prod(local.shape[1:])) * local.element_size()))
            return outer.real[0](local, n_total, group)

        def counts(local, cnt, group=None):
            outer.gathers.append((int(sum(cnt)), int(sum(cnt)) * int(np.prod(local.shape[1:])) * local.element_size()))
            return outer.real[1](local, cnt, group)

        def announce(self, op, ints=(), floats=()):
            outer.announced += 1
            return outer.real[2](self, op, ints, floats)
        sharded_db.all_gather_rows, sharded_db.all_gather_counts, cls._announce = rows, counts, announce

    def take(self):
        out = {"announcements": self.announced, "gathers": len(self.gathers), "gathered_bytes": sum(b for _n, b in self.gathers),
               "gathers_of_n_rows": sum(1 for n, _b in self.gathers if n > 64), "largest_gather_bytes": max([b for _n, b in self.gathers] or [0])}
        self.gathers, self.announced = [], 0
        return out

    def stop(self):
        self.mod.all_gather_rows, self.mod.all_gather_counts, self.cls._announce = self.real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000, help="clips")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    if args.repeats < 9:
        ap.error("at least 9 repeats")
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_sharded_bench: no GPU -- nothing is measured without one")
    from video_query_algorithms_amd import sharded_db
    from video_query_algorithms_amd.feature_store import save_store
    n, s, e, d, k = args.n, 2, 3, 1024, args.k
    rng = np.random.default_rng(17)
    x = np.abs(rng.standard_normal((n, s, e, d), dtype=np.float32)) * np.array([3.8, 1.2], dtype=np.float32).reshape(1, s, 1, 1)
    refs = [(37 * q + 1) % n for q in range(Q)]
    for ref in refs:                                 # relatives of every reference clip: the bands and the rankings are not empty
        rel = (ref + 3 + 5 * np.arange(60)) % n
        a = np.linspace(0.3, 0.98, 60, dtype=np.float32).reshape(-1, 1, 1, 1)
        x[rel] = a * x[ref] + (1 - a) * x[rel]
    rows = x[refs].astype(np.float64)
    targets = rows / (rows ** 2).sum(axis=-1, keepdims=True)
    weights = np.stack([[1.0, 0.6 + 0.1 * q] for q in range(Q)])
    bands = np.zeros((Q, 2))
    with tempfile.TemporaryDirectory() as tmp:
        store = save_store(os.path.join(tmp, "store"), x, np.arange(1, n + 1), ("rgb", "warped_optical_flow"), [1, 2, 3])
        db = sharded_db.ShardedFeatureDB.open(store, gpus=[0, 0], backend="gloo", batch_rounds=True)    # before this process's first GPU call
        traffic = _Traffic(sharded_db, sharded_db.ShardedFeatureDB)
        try:
            def own_rounds():
                return [db.query_round(targets[q], weights=weights[q], select=tuple(bands[q])) for q in range(Q)]

            def batched():
                r = db.query_round_batch(targets, weights, bands, want_avg=False, want_scores=False)
                return r, db.batch_round_topk(k)

            def timed(fn):
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out
            # review bands of a realistic size: the 40 best clips of every query match, the 60 behind them are near misses
            ranked_scores = [np.sort(db.query_round(targets[q], weights=weights[q]).scores) for q in range(Q)]
            bands[...] = [[0.5 * (v[-40] + v[-41]), 0.5 * (v[-100] + v[-101])] for v in ranked_scores]      # between two scores: no edge case
            for _ in range(3):
                own_rounds(), batched()
            traffic.take()
            a, b, worst, lists = [], [], 0.0, True
            for _ in range(args.repeats):
                ms, own = timed(own_rounds)
                a.append(ms)
                t_a = traffic.take()
                ms, (rounds, ranked) = timed(batched)
                b.append(ms)
                t_b = traffic.take()
                for q in range(Q):
                    order = np.lexsort((np.arange(n), -own[q].scores))[:k]
                    worst = max(worst, float(np.abs(np.asarray(ranked[q][1]) - own[q].scores[order]).max()))
                    lists = lists and len(rounds[q].match_rows) > 0 and len(rounds[q].match_rows) == len(own[q].match_rows)
            sa, sb = _stats(a), _stats(b)
            print(json.dumps({"n": n, "S": s, "E": e, "D": d, "world": 2, "backend": "gloo", "ranks_on_one_card": True, "tickets": Q, "k": k,
                              "repeats": args.repeats, "a_own_rounds_ms": sa, "b_batched_round_and_topk_ms": sb,
                              "a_over_b": round(sa["median"] / sb["median"], 2), "a_traffic": t_a, "b_traffic": t_b,
                              "ranked_values_max_abs_diff": worst, "match_counts_equal_and_not_empty": bool(lists)}), flush=True)
        finally:
            traffic.stop()
            db.close()


if __name__ == "__main__":
    main()
