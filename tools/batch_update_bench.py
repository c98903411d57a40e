"""The weight update of 16 tickets (12 revise, 4 finalize) behind one batched pass over a resident database: the two-call path
(batch_round_fit, the pick on the host, batch_round_rescore, and every finalize ticket's own select) against the one-call path
(batch_round_update: compute_similarities_batch(..., fit_on_device=True)).

    python tools/batch_update_bench.py [--n 10000] [--repeats 9]

Seeded and synthetic; fails when there is no GPU.  One process, after warm-up, the forms ALTERNATING (a repeat = form (a), then form
(b), then the pass alone), so drift of the shared host hits all alike; the host clock runs around a whole form, whose last device call
ends in its own synchronise.  Every form starts with the same pass over the 16 tickets; (a) and (b) end with every ticket's review set:

    (a)  compute_similarities_batch(fit=[True] * 16), then per ticket the fitted weights, compute_scores, the review budget
         (a finalize ticket: lowest_scoring_user_match), select_clips_to_review
    (b)  the same with fit_on_device=True

An update's time is its form's median minus the median of the pass alone.  The library calls of a form are counted where FeatureDB
makes them; the bytes the group's calls copy back and their kernel launches follow from the layouts (include/vq_amd_round_fit.h,
include/vq_amd_round_update.h) and are stated for pieces of at most 16 384 rows (the one-workgroup partition).  Every query is made
from a clip of the database; every ticket has 20 labelled clips (the 20 best of its query: the first 10 confirmed, the others
rejected), its own hyperparameters object with the reference's 40 x 31 grids, and looks ahead with a band at the 0.9995 / 0.999
quantiles of its scores.  One JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("COMPUTE_EPS", "0.000003")
import numpy as np

Q, G, T, PREFIX = 16, 40, 31, 1024
FINALIZE = (3, 7, 11, 15)
STREAMS = ("rgb", "warped_optical_flow")


def _stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


class _Target:
    def __init__(self, vectors, splits):
        self.target_features = {st: {sp: vectors[s, e].tolist() for e, sp in enumerate(splits)} for s, st in enumerate(STREAMS)}


def bench(vqa, n, e, repeats, warmup=2):
    # the modules whose library calls are counted: the handle's own and the one that makes the batched-round calls
    mods = {sys.modules[m] for m in (vqa.FeatureDB.__module__, vqa.FeatureDB.batch_round_update.__module__)}
    from video_query_algorithms_amd.compute_matches import _review_budget
    from video_query_algorithms_amd.ticket import compute_similarities_batch
    s, d = 2, 1024
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=17, scales=(4.0, 1.0))
    splits = list(range(1, e + 1))
    db.stream_names, db.slot_splits = list(STREAMS), [splits] * s
    t = np.stack([db.set_query_from_row((37 + 601 * q) % n) for q in range(Q)])      # every query is made from a clip of the database
    default = {"rgb": 1.0, "warped_optical_flow": 1.5}
    probe = db.scan_batch(t, np.tile([1.0, 1.5], (Q, 1)))
    ids = np.asarray(db.clip_ids)
    kinds = ["finalize" if q in FINALIZE else "revise" for q in range(Q)]
    tickets, hps, bands, labels = [], [], [], []
    for q in range(Q):
        th, lower = float(np.quantile(probe[q], 0.9995)), float(np.quantile(probe[q], 0.999))
        bands.append((th, (th - lower) / (1 - th)))                             # default threshold, near_miss_default: the look-ahead band
        best = np.argsort(-probe[q], kind="stable")[:20]
        matches = [{"video_clip": int(ids[r]), "user_match": bool(i < 10), "is_match": bool(i < 10)} for i, r in enumerate(best)]
        tk = vqa.Ticket({"query_id": q, "video_id": 1, "ref_clip": 0, "ref_clip_id": None, "search_set": None, "matches": matches,
                         "number_of_matches_to_review": 20, "user_matches": {str(int(ids[r])): True for r in best[:10]}}, feature_db=db)
        tk.target = _Target(t[q], splits)
        labels.append(matches)
        tickets.append(tk)
        hps.append(vqa.Hyperparameter(default, th, 0.3, bands[-1][1], 0.0, STREAMS, "global_pool", 1, 0.7, "bagging", 3))
    del probe
    calls = []
    real_call = vqa._lib.call

    def counting(name, *a):
        calls.append(name)
        return real_call(name, *a)

    def reset():
        for tk, hp, (th, _near), matches in zip(tickets, hps, bands, labels):
            hp.weights, hp.threshold = {}, th
            tk.matches = list(matches)                                        # the labels: select_clips_to_review replaces them by the review set
        random.seed(a=7)

    def form(**kw):
        reset()
        t0 = time.perf_counter()
        compute_similarities_batch(tickets, hps, **kw)
        if kw:
            for kind, tk, hp in zip(kinds, tickets, hps):
                hp.weights, hp.threshold = tk._fit
                tk.compute_scores(hp.weights)
                budget, reach = _review_budget(kind, tk, hp)
                tk.select_clips_to_review(hp.threshold, budget, reach)
        return (time.perf_counter() - t0) * 1e3

    two = {"fit": [True] * Q}
    one = {"fit": [True] * Q, "fit_on_device": True, "finalize": [k == "finalize" for k in kinds]}
    for _ in range(warmup):
        form(**two), form(**one), form()
    a, b, c, same, within = [], [], [], True, 0.0
    for m in mods:
        m.call = counting
    try:
        for _ in range(repeats):
            del calls[:]
            a.append(form(**two))
            calls_a = list(calls)
            got_a = [(hp.weights["warped_optical_flow"], hp.threshold, list(tk.matches.items())) for tk, hp in zip(tickets, hps)]
            del calls[:]
            b.append(form(**one))
            calls_b = list(calls)
            got_b = [(hp.weights["warped_optical_flow"], hp.threshold, list(tk.matches.items())) for tk, hp in zip(tickets, hps)]
            same = same and got_a == got_b
            within = max([within] + [abs(x[i] - y[i]) / abs(x[i]) for x, y in zip(got_a, got_b) for i in (0, 1)])
            lists = [len(tk._ahead["match_rows"]) + len(tk._ahead["near_rows"]) for tk in tickets]
            c.append(form())
    finally:
        for m in mods:
            m.call = real_call
    db.close()
    pass_calls = ["vq_db_query_round_batch"]
    behind = lambda names: [x for x in names if x not in pass_calls and x != "vq_host_alloc"]        # noqa: E731
    lists_back = Q * (32 + 2 * PREFIX * 8)                                      # results and the two prefixes of 16 queries
    sa, sb, sc = _stats(a), _stats(b), _stats(c)
    spread_a = sa["max"] - sa["min"]
    return {"n": n, "S": s, "E": e, "D": d, "tickets": Q, "finalize_tickets": len(FINALIZE), "labels_per_ticket": 20, "repeats": repeats,
            "a_two_calls_ms": sa, "b_one_call_ms": sb, "pass_alone_ms": sc,
            "a_update_ms": round(sa["median"] - sc["median"], 4), "b_update_ms": round(sb["median"] - sc["median"], 4),
            "a_spread_ms": round(spread_a, 4), "b_faster_than_a_by_more_than_the_spread": bool(sa["median"] - sb["median"] > spread_a),
            "a_library_calls_behind_the_pass": behind(calls_a), "b_library_calls_behind_the_pass": behind(calls_b),
            "a_group_bytes_back": Q * G * T * 8 + Q * n * 8 + lists_back, "b_group_bytes_back": Q * (64 + 16) + Q * n * 8 + lists_back,
            "a_group_launches": {"kernels": 3, "memsets": 1, "synchronisations": 2}, "b_group_launches": {"kernels": 5, "memsets": 1, "synchronisations": 1},
            "same_weights_thresholds_and_review_sets": bool(same), "largest_relative_difference_of_a_pick": float(within),
            "selected_rows_per_ticket": [min(lists), max(lists)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000, help="clips (at most 16384: the stated launches are those of short pieces)")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not 1000 <= args.n <= 16384:
        ap.error("1000 to 16384 clips")
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_update_bench: no GPU -- nothing is measured without one")
    import video_query_algorithms_amd as vqa
    print(json.dumps(bench(vqa, args.n, 3, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
