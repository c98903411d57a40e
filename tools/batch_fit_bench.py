"""The weight update of 16 revise tickets behind one batched pass: every ticket's own optimize_weights / compute_scores /
select_clips_to_review against the group's batch_round_fit + batch_round_rescore (ticket.compute_similarities_batch(..., fit=...)).

    python tools/batch_fit_bench.py [--n 1000000] [--repeats 9]

Seeded and synthetic; fails when there is no GPU.  One process, after warm-up, the two forms ALTERNATING (a repeat = form (a), then form
(b)), so drift of the shared host hits both alike; the host clock runs around a whole form, whose last device call ends in its own
synchronise.  Both forms start with the same compute_similarities_batch over the 16 tickets and end with every ticket's review set:

    (a)  compute_similarities_batch, then per ticket optimize_weights, compute_scores(weights), select_clips_to_review
    (b)  compute_similarities_batch(fit=[True] * 16), then per ticket the fitted weights, compute_scores, select_clips_to_review

Every query is made from a clip of the database; every ticket has 20 labelled clips (the 20 best of its query: the first 10 confirmed, the others rejected), its own hyperparameters
object with the reference's 40 x 31 grids, and looks ahead with a band at the 0.9995 / 0.999 quantiles of its scores.  Without --n the
two recorded shapes run: the 10 000-clip shape (10k x 2 x 3 x 1024 fp32, rows) and BASELINE cfg 4 (1M x 2 x 5 x 1024 fp32, tiled).  One
JSON line per shape.
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

Q = 16
STREAMS = ("rgb", "warped_optical_flow")


def _stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


class _Target:
    def __init__(self, vectors, splits):
        self.target_features = {st: {sp: vectors[s, e].tolist() for e, sp in enumerate(splits)} for s, st in enumerate(STREAMS)}


def bench(vqa, n, e, layout, repeats, warmup=2):
    from video_query_algorithms_amd.ticket import compute_similarities_batch
    s, d = 2, 1024
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=17, scales=(4.0, 1.0))
    if layout == "tiled":
        db.set_layout("tiled")
    splits = list(range(1, e + 1))
    db.stream_names, db.slot_splits = list(STREAMS), [splits] * s
    t = np.stack([db.set_query_from_row((37 + 601 * q) % n) for q in range(Q)])      # every query is made from a clip of the database
    default = {"rgb": 1.0, "warped_optical_flow": 1.5}
    probe = db.scan_batch(t, np.tile([1.0, 1.5], (Q, 1)))
    ids = np.asarray(db.clip_ids)
    tickets, hps, bands, labels = [], [], [], []
    for q in range(Q):
        th, lower = float(np.quantile(probe[q], 0.9995)), float(np.quantile(probe[q], 0.999))
        bands.append((th, (th - lower) / (1 - th)))                             # default threshold, near_miss_default: the look-ahead band
        best = np.argsort(-probe[q], kind="stable")[:20]
        matches = [{"video_clip": int(ids[r]), "user_match": bool(i < 10), "is_match": bool(i < 10)} for i, r in enumerate(best)]
        tk = vqa.Ticket({"query_id": q, "video_id": 1, "ref_clip": 0, "ref_clip_id": None, "search_set": None, "matches": matches,
                         "user_matches": {}}, feature_db=db)
        tk.target = _Target(t[q], splits)
        labels.append(matches)
        tickets.append(tk)
        hps.append(vqa.Hyperparameter(default, th, 0.3, bands[-1][1], 0.0, STREAMS, "global_pool", 1, 0.7, "bagging", 3))
    del probe

    def reset():
        for tk, hp, (th, _near), matches in zip(tickets, hps, bands, labels):
            hp.weights, hp.threshold = {}, th
            tk.matches = list(matches)                                        # the labels: select_clips_to_review replaces them by the review set
        random.seed(a=7)

    def finish(tk, hp):
        tk.compute_scores(hp.weights)
        tk.select_clips_to_review(hp.threshold, 20, hp.near_miss_default)

    def own():
        reset()
        t0 = time.perf_counter()
        compute_similarities_batch(tickets, hps)
        for tk, hp in zip(tickets, hps):
            hp.optimize_weights(tk)
            finish(tk, hp)
        return (time.perf_counter() - t0) * 1e3

    def fitted():
        reset()
        t0 = time.perf_counter()
        compute_similarities_batch(tickets, hps, fit=[True] * Q)
        for tk, hp in zip(tickets, hps):
            hp.weights, hp.threshold = tk._fit
            finish(tk, hp)
        return (time.perf_counter() - t0) * 1e3

    def pass_only():
        reset()
        t0 = time.perf_counter()
        compute_similarities_batch(tickets, hps)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        own(), fitted(), pass_only()
    a, b, c, same = [], [], [], True
    for _ in range(repeats):
        a.append(own())
        got_a = [(dict(hp.weights), hp.threshold, list(tk.matches.items())) for tk, hp in zip(tickets, hps)]
        b.append(fitted())
        same = same and got_a == [(dict(hp.weights), hp.threshold, list(tk.matches.items())) for tk, hp in zip(tickets, hps)]
        review = [len(tk.matches) for tk in tickets]
        lists = [len(tk._ahead["match_rows"]) + len(tk._ahead["near_rows"]) for tk in tickets]   # what the fitted bands select
        fitted_th = [float(hp.threshold) for hp in hps]
        c.append(pass_only())
    db.close()
    sa, sb, sc = _stats(a), _stats(b), _stats(c)
    spread_a = sa["max"] - sa["min"]
    return {"n": n, "S": s, "E": e, "D": d, "layout": layout, "tickets": Q, "labels_per_ticket": 20, "repeats": repeats,
            "a_pass_then_own_updates_ms": sa, "b_pass_then_group_fit_ms": sb, "pass_alone_ms": sc,
            "a_updates_ms": round(sa["median"] - sc["median"], 4), "b_updates_ms": round(sb["median"] - sc["median"], 4),
            "a_spread_ms": round(spread_a, 4), "b_faster_than_a_by_more_than_the_spread": bool(sa["median"] - sb["median"] > spread_a),
            "same_weights_thresholds_and_review_sets": bool(same), "review_set_sizes": [min(review), max(review)],
            "selected_rows_per_ticket": [min(lists), max(lists)], "fitted_thresholds": [round(min(fitted_th), 4), round(max(fitted_th), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="clips (default: the two recorded shapes)")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_fit_bench: no GPU -- nothing is measured without one")
    import video_query_algorithms_amd as vqa
    shapes = [(args.n, 5 if args.n >= 100_000 else 3, "tiled" if args.n >= 100_000 else "rows")] if args.n else [(10_000, 3, "rows"), (1_000_000, 5, "tiled")]
    for n, e, layout in shapes:
        print(json.dumps(bench(vqa, n, e, layout, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
