"""Test program (GPU box): the broker's side of a served ShardedFeatureDB with batched rounds.  Started by
tests/test_batch_sharded_gpu.py as a process of its own: ``ShardedFeatureDB.open(..., batch_rounds=True)`` starts the worker ranks
(shard_worker.py) and joins them as rank 0 -- every rank on the box's ONE card over gloo, or ONE rank over RCCL -- and the four calls
of a batched round, then ``compute_similarities_batch(fit=, top=)`` through the Ticket seam, run on the sharded database and on an
ordinary one-GPU FeatureDB over the same store.  Prints ``ok``; any difference is an assertion."""
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


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def same_partition(a, b):
    return same(a.match_rows, b.match_rows) and same(a.near_rows, b.near_rows) and a.near_argmax == b.near_argmax


def four_calls(one, sdb, refs):
    """The pass, the lean pass, the ranking, the fit and the re-weighting with len(refs) queries: sharded == one GPU."""
    n, S, Q = one.n, one.S, len(refs)
    t = np.stack([one.set_query_from_row(r) for r in refs])
    w = np.stack([[1.0, 0.5 + 0.125 * q] for q in range(Q)])
    plain = one.query_round_batch(t, w)
    ths = [float(np.sort(np.array(r.scores))[-(n // 4)]) for r in plain]
    bands = np.array([[th, th - 0.2] for th in ths])
    want = [(np.array(r.avg), np.array(r.n_e), np.array(r.scores), np.array(r.match_rows), np.array(r.near_rows), r.near_argmax)
            for r in one.query_round_batch(t, w, bands)]
    got = sdb.query_round_batch(t, w, bands)
    for q, (r, (avg, n_e, scores, match, near, am)) in enumerate(zip(got, want)):
        assert same(r.avg, avg) and same(r.n_e, n_e) and same(r.scores, scores), "query %d: the pass differs" % q
        assert same(r.match_rows, match) and same(r.near_rows, near) and r.near_argmax == am, "query %d: the partition differs" % q
    assert any(len(near) for _a, _n, _s, _m, near, _am in want) and any(len(match) for _a, _n, _s, match, _r, _am in want)
    # nothing N-sized back: the partitions (their near maxima read through batch_round_grid) and the ranking on what stayed on the cards
    lean = sdb.query_round_batch(t, w, bands, want_avg=False, want_scores=False)
    for q, (r, (_avg, _n_e, _scores, match, near, am)) in enumerate(zip(lean, want)):
        assert r.avg is None and r.scores is None
        assert same(r.match_rows, match) and same(r.near_rows, near) and r.near_argmax == am, "query %d: the lean partition differs" % q
    ks = [(3 + 7 * q) % (n + 4) + 1 for q in range(Q)]
    for q, ((rows, vals), (o_rows, o_vals)) in enumerate(zip(sdb.batch_round_topk(ks), one.batch_round_topk(ks))):
        assert same(rows, o_rows) and same(vals, o_vals), "query %d: the ranking differs" % q
    # the fit: labelled rows on every shard, a repeated row, an entry without labels, entries not in query order
    rng = np.random.default_rng(Q)
    hp = _vqa.Hyperparameter({"rgb": 1.0, "warped_optical_flow": 1.5})
    cand = np.zeros((len(hp.weight_grid), S))
    cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
    members = [[0], [1, 0], [Q - 1, 0, 1]][min(Q, 3) - 1]
    rows = [np.concatenate([[n - 1, 0, n // 2, 0], rng.integers(0, n, size=9)]), np.zeros(0, dtype=np.int64),
            np.array([22, 21, 32, 31, n - 1, 0])][:len(members)]                      # either side of the shard boundaries of 2 and 3 ranks
    labels = [(rng.random(r.size) < 0.4).astype(np.float64) for r in rows]
    args = (members, rows, labels, [cand] * len(members), [hp.threshold_grid] * len(members), [0.3] * len(members))
    for a, b, r in zip(sdb.batch_round_fit(*args), one.batch_round_fit(*args), rows):
        assert (a is None and b is None and r.size == 0) or (a.shape == (40, 31) and same(a, b)), "the loss surfaces differ"
    new_w = np.stack([[1.0, 2.25 - 0.125 * i] for i in range(len(members))])
    new_bands = np.array([[ths[q] - 0.05, ths[q] - 0.3] for q in members])
    for a, b in zip(sdb.batch_round_rescore(members, new_w, new_bands), one.batch_round_rescore(members, new_w, new_bands)):
        assert same(a.scores, b.scores) and same_partition(a, b), "the re-weighting differs"
    for (rows_a, vals_a), (rows_b, vals_b) in zip(sdb.batch_round_topk(6), one.batch_round_topk(6)):
        assert same(rows_a, rows_b) and same(vals_a, vals_b), "the ranking behind the re-weighting differs"


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
    random.seed(a=SEED)
    _vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, False, True, False], top=[5, 7, 64, 1])
    out = []
    for tk in tickets:
        weights, th = tk._fit if tk._fit is not None else (dict(DEFAULT_WEIGHTS), 0.8)
        tk.compute_scores(weights)
        tk.select_clips_to_review(th, tk.number_of_matches_to_review, hp.near_miss_default)
        out.append((tk._fit, list(tk.matches.items()), np.array(tk._top[0]), np.array(tk._top[1]), np.array(tk._ahead["scores"])))
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
            assert sdb.batch_round_supported() and one.batch_round_supported()
            four_calls(one, sdb, [1, 7, 30, 41, 63])
            four_calls(one, sdb, [12])
            four_calls(one, sdb, [(5 * q + 3) % 64 for q in range(16)])
            (got, r_got), (want, r_want) = ticket_rounds(sdb, g, ids, recs), ticket_rounds(one, g, ids, recs)
            assert got[0][0] is not None and got[2][0] is not None and got[1][0] is None and got[3][0] is None
            for (fit_a, m_a, tr_a, tv_a, sc_a), (fit_b, m_b, tr_b, tv_b, sc_b) in zip(got, want):
                assert fit_a == fit_b, (fit_a, fit_b)                              # the fitted (weights, threshold)
                assert m_a == m_b and len(m_a) > 0, "review sets differ"
                assert same(tr_a, tr_b) and same(tv_a, tv_b) and same(sc_a, sc_b), "rankings or look-ahead scores differ"
            assert r_got == r_want                                                  # the generator advanced identically
            one.close()
        finally:
            sdb.close()
        assert all(p.returncode == 0 for p in sdb._workers), [p.returncode for p in sdb._workers]
    print("ok", flush=True)


if __name__ == "__main__":
    main()
