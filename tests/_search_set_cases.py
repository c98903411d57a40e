"""Test infrastructure for search sets (row views of a resident database): the row lists every scan test walks, bitwise comparison,
numpy restatements of what runs behind the scan, and the two-ticket scenario shared by the GPU, gloo and stand-in tests."""
import random

import numpy as np


def bits(a):
    """float64 / int32 arrays as integers: NaN patterns compare like everything else."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def same_values(a, b):
    """Against numpy on the host: the same bits wherever the value is a number, NaN where it is NaN (the sign and payload of a NaN
    that an operation PRODUCES are the processor's choice)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def view_lists(n, seed=11):
    """name -> strictly ascending rows of a database of n clips."""
    rng = np.random.default_rng(seed)
    runs = np.concatenate([np.arange(a, min(a + 37, n)) for a in range(3, n, 37 + 11)])       # runs of 37 rows, gaps of 11
    out = {"empty": np.zeros(0, np.int64), "first": np.array([0]), "last": np.array([n - 1]), "identity": np.arange(n),
           "every_second": np.arange(0, n, 2), "runs": runs}
    out["random_half"] = np.sort(rng.choice(n, n // 2, replace=False))
    return {k: v.astype(np.int64) for k, v in out.items()}


def presence_mask(n, s, e, seed=5):
    """~80 % of the (clip, stream, split) slots present; clip 1 lacks stream 0 altogether, the last clip every slot of the last stream."""
    p = (np.random.default_rng(seed).random((n, s, e)) < 0.8).astype(np.uint8)
    p[1 % n, 0, :] = 0
    p[n - 1, s - 1, :] = 0
    return p


def np_topk(scores, k):
    """descending, ties by ascending position, NaNs excluded"""
    v = np.asarray(scores)
    idx = np.flatnonzero(~np.isnan(v))
    order = idx[np.lexsort((idx, -v[idx]))][:k]
    return order.astype(np.int64), v[order]


def tie_ks(scores, cap):
    """k in the middle of the best run of equal scores, at its end, one past it, and the same around the end of the third run"""
    vals, counts = np.unique(scores[~np.isnan(scores)], return_counts=True)
    if not counts.size:
        return []
    runs = counts[::-1]                                               # best value first
    ends = np.cumsum(runs)
    ks = [max(1, int(runs[0]) // 2), int(ends[0]), int(ends[0]) + 1]
    if len(ends) >= 3:
        ks += [int(ends[2]) - 1, int(ends[2]), int(ends[2]) + 1]
    return [k for k in ks if 1 <= k <= min(cap, scores.size)]


ROUND_PREFIX = 1024


def round_layout(Q, S, E, D, m=None, n=None):
    """(off[12], start[17]) of a batched round's block as the comments of include/vq_amd_rounds.h (``n``: a whole-database round,
    n_e once per database, off[11] = 0) and include/vq_amd_round_views.h (``m``: the rows of each query's piece, n_e once per piece,
    off[11] = sum M) state them: nine pieces, each rounded up to 64 bytes, then off[9] = their bytes, off[10] = P."""
    pieces = [n] * Q if m is None else list(m)
    start = [0]
    for q in range(16):
        start.append(start[-1] + (pieces[q] if q < Q else 0))
    sm = start[Q]
    P = ROUND_PREFIX
    sizes = [Q * S * E * D * 8, Q * 8 * 8, Q * 2 * 8, (n if m is None else sm) * S * 4, sm * S * 8, sm * 8, Q * 4 * 8, Q * P * 8, Q * P * 8]
    off = [0]
    for b in sizes:
        off.append(off[-1] + (b + 63) // 64 * 64)
    return off + [P, 0 if m is None else sm], start


def np_select(scores, th, lower):
    v = np.asarray(scores)
    with np.errstate(invalid="ignore"):
        match = np.flatnonzero(v >= th)
        near = np.flatnonzero((lower <= v) & (v < th))
    return match, near, (int(near[np.argmax(v[near])]) if near.size else -1)


def np_min_score(scores, rows):
    m = 1.0
    for r in rows:
        m = min(m, scores[r])
    return m


def host_loss_surface(graded, labels, th_grid, ballast):
    """The host route of Hyperparameter.optimize_weights (hyperparameter.py, the lines behind ``scores_grid``) on graded [G][L] scores:
    the sums BEFORE the division by the number of labels, which is what the device's loss surface returns."""
    th = np.asarray(th_grid)[None, :]
    surface = np.tile(0.5 * th, (graded.shape[0], 1))
    y = np.array([float(v) for v in labels], dtype=np.float64)[:, None, None]
    margin = graded.T[:, :, None] - th[None]
    terms = (np.heaviside(margin, 1) - y) * margin * (1 + y * ballast)
    for term in terms:
        surface = surface + term
    return surface


# ---------------------------------------------------------------------------------------------------------------------------------
# two tickets, two search sets, one resident database
# ---------------------------------------------------------------------------------------------------------------------------------
def ticket_round(vqa, db, recs, ref_clip_id, search_set, user_matches, labelled, streams, default_weights, seed, pause=None):
    """One query round of compute_matches.py:58-89 through the drop-in; ``pause(where)`` runs in every gap (another ticket's round)."""
    tk = vqa.Ticket({"query_id": 1, "video_id": 1, "ref_clip": 0, "ref_clip_id": int(ref_clip_id), "search_set": search_set,
                     "number_of_matches_to_review": 20, "dynamic_target_adjustment": False, "user_matches": dict(user_matches)},
                    records=recs, feature_db=db)
    hp = vqa.Hyperparameter(default_weights, 0.8, 0.1, 0.35, 0.0, streams, "global_pool", 1, 0.7, "bagging", 3)
    tk.target = vqa.TargetClip(tk, hp)
    tk.target.get_target_features()
    tk.compute_similarities(hp)
    if pause:
        pause("similarities")
    tk.compute_scores(default_weights)
    if pause:
        pause("scores")
    random.seed(a=seed)
    tk.select_clips_to_review(0.8, 6, 0.35)
    first = dict(tk.matches)
    low = tk.lowest_scoring_user_match()
    if pause:
        pause("review")
    tk.matches = labelled
    hp.optimize_weights(tk)
    if pause:
        pause("weights")
    tk.compute_scores(hp.weights)
    random.seed(a=seed)
    tk.select_clips_to_review(hp.threshold, 20, 0.35)
    return {"similarities": {c: v for c, v in tk.similarities.items()}, "scores_default": None, "scores": dict(tk.scores.items()),
            "first": first, "matches": dict(tk.matches), "lowest": low, "weights": dict(hp.weights), "threshold": hp.threshold}


def same_round(a, b):
    """dict equality INCLUDING order, values bit for bit"""
    def same_map(x, y):
        return list(x.keys()) == list(y.keys()) and all(same_bits(np.float64(x[k]), np.float64(y[k])) for k in x)
    sims_ok = list(a["similarities"].keys()) == list(b["similarities"].keys()) and all(
        list(a["similarities"][c].keys()) == list(b["similarities"][c].keys()) and all(
            same_bits(np.float64(a["similarities"][c][st][0]), np.float64(b["similarities"][c][st][0]))
            and a["similarities"][c][st][1] == b["similarities"][c][st][1] for st in a["similarities"][c]) for c in a["similarities"])
    return (sims_ok and same_map(a["scores"], b["scores"]) and same_map(a["first"], b["first"]) and same_map(a["matches"], b["matches"])
            and a["lowest"][1] == b["lowest"][1] and same_bits(np.float64(a["lowest"][0]), np.float64(b["lowest"][0]))
            and a["weights"] == b["weights"] and a["threshold"] == b["threshold"])


def two_ticket_plan(g, ids):
    """From the real_subset golden: set 'A' holds ticket A's reference clip, set 'B' does not hold ticket B's.  Returns
    {name: (search-set clip ids in a scrambled order with a duplicate, reference clip id, user_matches, labelled)}."""
    ids = [int(c) for c in ids]
    ref_a, ref_b = int(g["ref_clip_id"]), ids[3]
    set_a = [c for i, c in enumerate(ids) if i % 3 != 1 or c == ref_a]
    set_b = [c for i, c in enumerate(ids) if i % 4 != 0 and c != ref_b]

    def labelled(members):
        lab = [m for m in g["labelled"] if m["video_clip"] in members]
        assert len(lab) >= 4 and any(m["user_match"] for m in lab)
        return lab

    def confirmed(members):
        return {k: v for k, v in g["user_matches"].items() if int(k) in members}
    plan = {"A": (set_a[::-1] + set_a[:1], ref_a, confirmed(set_a), labelled(set_a)),
            "B": (set_b[1::2] + set_b[0::2], ref_b, confirmed(set_b), labelled(set_b))}
    assert ref_a in set_a and ref_b not in set_b
    return plan


def check_two_tickets(vqa, shared, make_alone, recs, x, ids, g, streams, default_weights, seed):
    """``shared``: ONE database holding all of ``x`` / ``ids``; ``make_alone(rows)``: a database of only those rows (the path the
    reference's goldens pin).  Each ticket alone on its own database, then A's round with B's whole round in every gap -- and B's
    with A's -- on the shared one: dict for dict the same."""
    ids = np.asarray(ids, dtype=np.int64)
    plan = two_ticket_plan(g, ids)
    alone = {}
    for name, (members, ref, um, lab) in plan.items():
        rows = np.unique([int(np.flatnonzero(ids == c)[0]) for c in members])
        own = make_alone(rows)
        sub = [r for r in recs if r["video_clip_id"] in set(members) or r["video_clip_id"] == ref]
        alone[name] = ticket_round(vqa, own, sub, ref, name, um, lab, streams, default_weights, seed)
        own.close()
        view = shared.define_search_set(name, members)
        assert (view.rows == rows).all() and (view.clip_ids == ids[rows]).all() and view.n == rows.size
        assert list(alone[name]["scores"].keys()) == ids[rows].tolist()
        assert (ref in alone[name]["matches"]) == (name == "A")               # the reference clip is forced in only where it is searched

    def run(name, pause=None):
        members, ref, um, lab = plan[name]
        return ticket_round(vqa, shared, recs, ref, name, um, lab, streams, default_weights, seed, pause=pause)
    for first, other in (("A", "B"), ("B", "A")):
        seen = []

        def intruder(where, other=other):
            seen.append(where)
            state = random.getstate()
            assert same_round(run(other), alone[other]), ("intruder %s after %s" % (other, where))
            random.setstate(state)
        assert same_round(run(first, pause=intruder), alone[first]), "round of %s interleaved with %s" % (first, other)
        assert seen == ["similarities", "scores", "review", "weights"]
    # a confirmed match outside the ticket's search set: KeyError, as at ticket.py:355
    members, ref, um, lab = plan["B"]
    outside = next(int(c) for c in ids if int(c) not in set(members))
    tk = vqa.Ticket({"query_id": 1, "video_id": 1, "ref_clip": 0, "ref_clip_id": ref, "search_set": "B", "user_matches": {str(outside): True}},
                    records=recs, feature_db=shared)
    hp = vqa.Hyperparameter(default_weights, 0.8, 0.1, 0.35, 0.0, streams, "global_pool", 1, 0.7, "bagging", 3)
    tk.target = vqa.TargetClip(tk, hp)
    tk.target.get_target_features()
    tk.compute_similarities(hp)
    tk.compute_scores(default_weights)
    assert outside not in tk.scores and len(tk.scores) == len(set(members))
    try:
        tk.select_clips_to_review(0.8, 20, 0.35)
    except KeyError:
        pass
    else:
        raise AssertionError("a confirmed match outside the search set must be a KeyError")
    shared.use_search_set(None)
    for name in plan:
        shared.drop_search_set(name)
