"""16 query rounds one after the other against ONE batched round of the same 16 (FeatureDB.query_round vs query_round_batch).

    python tools/batch_round_bench.py [--n 1000000] [--repeats 7]

Seeded and synthetic; fails when there is no GPU.  One process, after warm-up, the forms ALTERNATING (a repeat = form (a), then form
(b), then the plain scan_batch pass between two HIP events), so drift of the shared host hits all alike.  Forms (a) and (b) end in
their own synchronise: the host clock stops after the last result is on the host.  Without --n the two recorded shapes run: BASELINE
cfg 4 (1M x 2 x 5 x 1024 fp32, tiled) and the 10 000-clip shape (10k x 2 x 3 x 1024 fp32, rows).  One JSON line per shape.

    python tools/batch_round_bench.py --sets [--n 1000000] [--repeats 9]

Rounds under search sets: ONE view round (FeatureDB.query_round_batch_sets) against the same tickets' one-query rounds under
use_search_set, one after the other, alternating as above.  Four groups per database: 16 queries on one 10 % set (runs of 100 rows), 16
on two 50 % sets that overlap by half, 16 whole-database queries (against query_round_batch: the cost of the view form itself) and a
group exactly at sum M = 2 x distinct (two queries on one 10 % set).  Without --n: 1M x 2 x 5 x 1024 fp32 in rows and tiled layout and
10 000 x 2 x 3 x 1024 rows.  One JSON line per database.
"""
import argparse
import ctypes as C
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


def bench(vqa, n, s, e, d, layout, repeats, warmup=2):
    from video_query_algorithms_amd._lib import call
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=17, scales=(4.0, 1.0)[:s])
    if layout == "tiled":
        db.set_layout("tiled")
    rng = np.random.default_rng(0)
    t = rng.standard_normal((Q, s, e, d)) / d
    w = 0.5 + rng.random((Q, s))
    probe = db.scan_batch(t, w)
    bands = np.array([[np.quantile(probe[q], 0.9995), np.quantile(probe[q], 0.999)] for q in range(Q)])   # review-sized lists: inside the prefix
    del probe

    def sequential():
        t0 = time.perf_counter()
        for q in range(Q):
            db.query_round(t[q], w[q], (bands[q, 0], bands[q, 1]))          # returns after its own synchronise
        return (time.perf_counter() - t0) * 1e3

    def batched():
        t0 = time.perf_counter()
        db.query_round_batch(t, w, bands, want_avg=True, timed=True)        # returns after its own synchronise
        return (time.perf_counter() - t0) * 1e3, db.batch_round_times()

    tm = C.c_void_p()
    call("vq_timer_create", C.byref(tm))

    def plain_pass():                                                       # device time between two events around the launch
        call("vq_timer_start", tm, None)
        db.scan_batch(t, w, want=False)
        call("vq_timer_stop", tm, None)
        ms = C.c_float()
        call("vq_timer_elapsed_ms", tm, C.byref(ms))
        return ms.value

    for _ in range(warmup):
        sequential(), batched(), plain_pass()
    seq, bat, split, plain = [], [], [], []
    for _ in range(repeats):
        seq.append(sequential())
        ms, parts = batched()
        bat.append(ms)
        split.append(parts)
        plain.append(plain_pass())
    call("vq_timer_destroy", tm)
    db.close()
    a, b = _stats(seq), _stats(bat)
    spread_a = a["max"] - a["min"]
    return {"n": n, "S": s, "E": e, "D": d, "layout": layout, "queries": Q, "repeats": repeats,
            "a_16_query_rounds_ms": a, "a_per_round_ms": {k: round(v / Q, 4) for k, v in a.items()},
            "b_one_batched_round_ms": b, "b_per_round_ms": {k: round(v / Q, 4) for k, v in b.items()},
            "b_split_ms": {name: _stats([p[i] for p in split]) for i, name in enumerate(("pass", "selection", "copy_back"))},
            "scan_batch_pass_ms": _stats(plain),
            "a_spread_ms": round(spread_a, 4), "b_faster_than_a_by_more_than_the_spread": bool(a["median"] - b["median"] > spread_a)}


def bench_sets(vqa, n, s, e, d, layout, repeats, warmup=2):
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=17, scales=(4.0, 1.0)[:s])
    if layout == "tiled":
        db.set_layout("tiled")
    rows = np.arange(n, dtype=np.int64)
    db.define_search_rows("tenth", rows[rows % 1000 < 100])
    db.define_search_rows("half_a", rows[:n // 2])
    db.define_search_rows("half_b", rows[n // 4:n // 4 + n // 2])
    rng = np.random.default_rng(0)
    t = rng.standard_normal((Q, s, e, d)) / d
    w = 0.5 + rng.random((Q, s))
    probe = db.scan_batch(t, w)
    bands = np.array([[np.quantile(probe[q], 0.9995), np.quantile(probe[q], 0.999)] for q in range(Q)])
    del probe
    groups = {"one_tenth_set_x16": ["tenth"] * Q, "two_half_sets_x8": ["half_a", "half_b"] * (Q // 2), "whole_x16": [None] * Q,
              "at_the_rule_2x_one_tenth": ["tenth"] * 2}

    def solo(ids):
        t0 = time.perf_counter()
        for q, sid in enumerate(ids):
            db.use_search_set(sid)
            db.query_round(t[q], w[q], (bands[q, 0], bands[q, 1]))
        return (time.perf_counter() - t0) * 1e3

    def shared(ids):
        k = len(ids)
        t0 = time.perf_counter()
        db.query_round_batch_sets(t[:k], w[:k], ids, bands[:k], want_avg=True, timed=True)
        return (time.perf_counter() - t0) * 1e3, db.batch_round_times()

    def whole_batch():
        t0 = time.perf_counter()
        db.use_search_set(None)
        db.query_round_batch(t, w, bands, want_avg=True, timed=True)
        return (time.perf_counter() - t0) * 1e3, db.batch_round_times()

    out = {"n": n, "S": s, "E": e, "D": d, "layout": layout, "repeats": repeats, "groups": {}}
    for name, ids in groups.items():
        for _ in range(warmup):
            solo(ids), shared(ids)
        a, b, split, c, csplit = [], [], [], [], []
        for _ in range(repeats):
            a.append(solo(ids))
            ms, parts = shared(ids)
            b.append(ms)
            split.append(parts)
            if name == "whole_x16":
                ms, parts = whole_batch()
                c.append(ms)
                csplit.append(parts)
        union = db.last_view_round_union
        sa, sb = _stats(a), _stats(b)
        g = {"queries": len(ids), "sum_m": int(sum(n if i is None else db.search_set_view(i).n for i in ids)), "union_rows": union[0],
             "union_tiles": union[1], "solo_rounds_ms": sa, "view_round_ms": sb,
             "view_round_split_ms": {k: _stats([p[i] for p in split]) for i, k in enumerate(("plan_pass_ne", "selection", "copy_back"))},
             "solo_spread_ms": round(sa["max"] - sa["min"], 4), "view_round_wins": bool(sb["median"] < sa["median"])}
        if c:
            sc = _stats(c)
            g["query_round_batch_ms"] = sc
            g["query_round_batch_split_ms"] = {k: _stats([p[i] for p in csplit]) for i, k in enumerate(("pass", "selection", "copy_back"))}
            g["view_form_slower_than_batch_by_more_than_the_spread"] = bool(sb["median"] - sc["median"] > sc["max"] - sc["min"])
        out["groups"][name] = g
    db.use_search_set(None)
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="clips (default: the two recorded shapes)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sets", action="store_true", help="rounds under search sets: one view round against the one-query rounds")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_round_bench: no GPU -- nothing is measured without one")
    import video_query_algorithms_amd as vqa
    if args.sets:
        e = 5 if (args.n or 1_000_000) >= 100_000 else 3
        shapes = [(args.n, 2, e, 1024, "rows"), (args.n, 2, e, 1024, "tiled")] if args.n else [(1_000_000, 2, 5, 1024, "rows"), (1_000_000, 2, 5, 1024, "tiled"),
                                                                                              (10_000, 2, 3, 1024, "rows")]
        for n, s, e, d, layout in shapes:
            print(json.dumps(bench_sets(vqa, n, s, e, d, layout, max(args.repeats, 9))), flush=True)
        return
    shapes = [(args.n, 2, 5, 1024, "tiled" if args.n >= 100_000 else "rows")] if args.n else [(1_000_000, 2, 5, 1024, "tiled"), (10_000, 2, 3, 1024, "rows")]
    for n, s, e, d, layout in shapes:
        print(json.dumps(bench(vqa, n, s, e, d, layout, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
