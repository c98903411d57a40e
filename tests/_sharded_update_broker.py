"""Test program (GPU box): the broker's side of a served ShardedFeatureDB whose groups update their weights in ONE operation.  Started by
tests/test_batch_update_sharded_gpu.py as a process of its own: ``ShardedFeatureDB.open(..., batch_rounds=True)`` starts the worker
ranks (shard_worker.py) and joins them as rank 0 -- every rank on the box's ONE card over gloo, or ONE rank over RCCL -- and
``batch_round_update``, the ranking behind it, then ``compute_similarities_batch(fit=, fit_on_device=True, finalize=, top=)`` through
the Ticket seam, run on the sharded database and on an ordinary one-GPU FeatureDB over the same store.  Prints ``ok``; any difference
is an assertion."""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("COMPUTE_EPS", "0.000003")

FIELDS = ("w", "threshold", "lowest", "iw", "it", "on_rim", "fell_back", "near_argmax")


def bits(a, b):
    """== on bit patterns (None only equals None)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def rows_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def kept(r):
    """A result's values, out of the pooled block the next call may take."""
    copy = lambda v: None if v is None else np.array(v)                       # noqa: E731
    return {"scores": copy(r.scores), "match_rows": copy(r.match_rows), "near_rows": copy(r.near_rows), "surface": copy(r.surface),
            "band": None if r.band is None else tuple(float(v) for v in r.band), "avg": copy(r.avg), "n_e": copy(r.n_e),
            **{f: (None if getattr(r, f) is None else getattr(r, f) if isinstance(getattr(r, f), (bool, int)) else float(getattr(r, f))) for f in FIELDS}}


def same_update(a, b, what, scores=True):
    assert all(bits(a[f], b[f]) if isinstance(b[f], float) else a[f] == b[f] for f in FIELDS), (what, [(a[f], b[f]) for f in FIELDS])
    assert bits(a["band"], b["band"]), (what, a["band"], b["band"])
    assert rows_equal(a["match_rows"], b["match_rows"]) and rows_equal(a["near_rows"], b["near_rows"]), "%s: the partition differs" % what
    assert bits(a["avg"], b["avg"]) and rows_equal(a["n_e"], b["n_e"]), "%s: the round's own similarities differ" % what
    if scores:
        assert bits(a["scores"], b["scores"]), "%s: the scores differ" % what
        assert bits(a["surface"], b["surface"]), "%s: the loss surface differs" % what
    else:
        assert a["scores"] is None and a["surface"] is None


def update_calls(one, sdb, refs):
    """A round of len(refs) >= 5 queries, then the whole weight update of five of them: sharded == one GPU."""
    n, S, Q = one.n, one.S, len(refs)
    t = np.stack([one.set_query_from_row(r) for r in refs])
    w = np.stack([[1.0, 0.5 + 0.125 * q] for q in range(Q)])
    bands = np.array([[0.8, 0.6]] * Q)
    scores = [np.array(r.scores) for r in one.query_round_batch(t, w, bands)]
    sdb.query_round_batch(t, w, bands)
    hp = _vqa.Hyperparameter({"rgb": 1.0, "warped_optical_flow": 1.5})
    cand = np.zeros((len(hp.weight_grid), S))
    cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
    rng = np.random.default_rng(Q)
    # not in query order; rows either side of the shard boundaries of 2 and 3 ranks, row 0 twice; an entry without labels between served
    # ones; a revise member; finalize members whose user rows sit on the last rank only, on every rank, nowhere
    members = [Q - 1, 0, 3, 1, 2]
    best = np.argsort(-scores[2])[:24]
    rows = [np.concatenate([[22, 21, 32, 31, n - 1, 0, n // 2, 0], rng.integers(0, n, size=9)]), np.zeros(0, dtype=np.int64),
            np.concatenate([[43, 42, 1], rng.integers(0, n, size=8)]), np.array([5, 31, n - 1, 5]), best]
    labels = [(rng.random(r.size) < 0.4).astype(np.float64) for r in rows]
    labels[4] = np.array([float(bool(scores[2][r] >= scores[2][best[12]]) ^ bool(rng.random() < 0.12)) for r in best])
    users = [[], [], [50, 57, n - 1], [], [0, 21, 22, 40, n - 1]]
    reaches = [hp.near_miss_default, hp.near_miss_default, None, None, None]
    k = len(members)
    args = (members, rows, labels, [cand] * k, [hp.threshold_grid] * k, [hp.ballast] * k, [1] * k, float(os.environ["COMPUTE_EPS"]), reaches, users)
    want = [kept(r) for r in one.batch_round_update(*args, want_surface=True)]
    got = [kept(r) for r in sdb.batch_round_update(*args, want_surface=True)]
    for i, (a, b) in enumerate(zip(got, want)):
        same_update(a, b, "entry %d (query %d)" % (i, members[i]))
    assert want[1]["w"] is None and want[1]["scores"] is None and all(b["w"] is not None for i, b in enumerate(want) if i != 1)
    assert want[3]["lowest"] == 1.0 and want[2]["lowest"] < 1.0 and want[4]["lowest"] < 1.0
    served = [q for i, q in enumerate(members) if i != 1]
    ks = [3 + 5 * j for j in range(len(served))]
    for q, ((rows_a, vals_a), (rows_b, vals_b)) in zip(served, zip(sdb.batch_round_topk(ks, served), one.batch_round_topk(ks, served))):
        assert rows_equal(rows_a, rows_b) and bits(vals_a, vals_b), "query %d: the ranking behind the update differs" % q
    # the scores stay on the cards: the partitions (their near maxima read through batch_round_grid) and the ranking still agree
    sdb.query_round_batch(t, w, bands, want_avg=True, want_scores=False)
    lean = [kept(r) for r in sdb.batch_round_update(*args, want_scores=False)]
    for i, (a, b) in enumerate(zip(lean, want)):
        same_update(a, b, "lean entry %d" % i, scores=False)
    for q, ((rows_a, vals_a), (rows_b, vals_b)) in zip(served, zip(sdb.batch_round_topk(ks, served), one.batch_round_topk(ks, served))):
        assert rows_equal(rows_a, rows_b) and bits(vals_a, vals_b), "query %d: the ranking behind the lean update differs" % q


def ticket_rounds(db, g, ids, recs):
    from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS
    hp = _vqa.Hyperparameter(DEFAULT_WEIGHTS, 0.8, g["ballast"], 0.35, 0.3, STREAMS, "global_pool", 1, 0.7, "bagging", 3)
    tickets = []
    for ref, labelled in ((g["ref_clip_id"], True), (int(ids[7]), False), (int(ids[40]), True), (int(ids[63]), False)):
        tk = _vqa.Ticket({"query_id": 1, "video_id": 1, "ref_clip": 0, "ref_clip_id": ref, "search_set": 1, "number_of_matches_to_review": 20,
                          "matches": g["labelled"] if labelled else [], "user_matches": g["user_matches"] if labelled else {}},
                         records=recs, feature_db=db)
        tk.target = _vqa.TargetClip(tk, hp)
        tk.target.get_target_features()
        tickets.append(tk)
    finalize = [False, False, True, False]
    random.seed(a=SEED)
    _vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, False, True, False], fit_on_device=True, finalize=finalize, top=[5, 7, 64, 1])
    out = []
    for tk, fin in zip(tickets, finalize):
        weights, th = tk._fit if tk._fit is not None else (dict(DEFAULT_WEIGHTS), 0.8)
        tk.compute_scores(weights)
        budget, reach = tk.number_of_matches_to_review, hp.near_miss_default
        if fin:                                                               # compute_matches._review_budget
            lowest, _clip = tk.lowest_scoring_user_match()
            budget, reach = float("inf"), max(th - lowest, 0) / max(1 - th, float(os.environ["COMPUTE_EPS"]))
        tk.select_clips_to_review(th, budget, reach)
        out.append((tk._fit, list(tk.matches.items()), np.array(tk._top[0]), np.array(tk._top[1]), np.array(tk._ahead["scores"]), tk._ahead["select"]))
    return out, random.random()


def main():
    global _vqa
    world, backend = int(sys.argv[1]), sys.argv[2]
    import video_query_algorithms_amd as _vqa
    from video_query_algorithms_amd.feature_store import save_store
    from video_query_algorithms_amd.sharded_db import ShardedFeatureDB
    from _helpers import STREAMS, golden_json, golden_npy, records_from_dense
    g = golden_json("synth_small.json")
    x = golden_npy("synth_small_x.npy")
    ids = np.asarray(g["clip_order"])
    recs = records_from_dense(x, ids, [1, 2, 3])
    with tempfile.TemporaryDirectory() as d:
        store = save_store(os.path.join(d, "store"), x, ids, STREAMS, [1, 2, 3])
        sdb = ShardedFeatureDB.open(store, gpus=[0] * world, backend=backend, batch_rounds=True)      # before this process's first GPU call
        try:
            one = _vqa.FeatureDB.from_store(store)
            assert sdb.batch_round_supported() and one.batch_round_supported() and hasattr(sdb, "batch_round_update")
            update_calls(one, sdb, [1, 7, 30, 41, 63])
            update_calls(one, sdb, [(5 * q + 3) % 64 for q in range(16)])
            (got, r_got), (want, r_want) = ticket_rounds(sdb, g, ids, recs), ticket_rounds(one, g, ids, recs)
            assert got[0][0] is not None and got[2][0] is not None and got[1][0] is None and got[3][0] is None
            for (fit_a, m_a, tr_a, tv_a, sc_a, band_a), (fit_b, m_b, tr_b, tv_b, sc_b, band_b) in zip(got, want):
                assert fit_a == fit_b, (fit_a, fit_b)                              # the fitted (weights, threshold)
                assert band_a == band_b and m_a == m_b and len(m_a) > 0, "review bands or review sets differ"
                assert rows_equal(tr_a, tr_b) and bits(tv_a, tv_b) and bits(sc_a, sc_b), "rankings or look-ahead scores differ"
            assert r_got == r_want                                                  # the generator advanced identically
            one.close()
        finally:
            sdb.close()
        assert all(p.returncode == 0 for p in sdb._workers), [p.returncode for p in sdb._workers]
    print("ok", flush=True)


if __name__ == "__main__":
    main()
