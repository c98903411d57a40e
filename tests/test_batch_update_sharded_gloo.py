"""CPU, 2-3 processes over gloo: ShardedFeatureDB.batch_round_update -- a group's whole weight update on a row-sharded database as ONE
operation -- against FeatureDB.batch_round_update's stand-in on the unsharded rows (tests/_standin_update.py), everything with == (bit
patterns where a NaN occurs).

Every rank's "kernels" are the numpy stand-in of tests/_standin_shard_update.py, so under test is what ShardedFeatureDB adds: the one
announcement, the tables of the labelled and the user rows' averaged similarities put together by ONE all-reduce of bit patterns, the
same local call on every rank, the one gather of the scores and the two small gathers of the partitions, the error agreement -- and
ticket.compute_similarities_batch(fit_on_device=True) / compute_matches(fit_weights="device") on top of it.  The GPU twin is
tests/test_batch_update_sharded_gpu.py."""
import os
import random
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from test_batch_sharded_gloo import _Gathers, _port, _same, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, E, D, N = 2, 3, 64, 64
SNAN = np.array([0x7FF0000000000123], dtype=np.uint64).view(np.float64)[0]       # a signalling NaN with a payload: x + 0.0 would quiet it


def _bits(a, b):
    """== on the bit patterns of two float arrays or scalars (None only equals None)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def _databases(x, ids, served, batch_rounds=True, planted=None):
    """(the sharded database of this rank, the unsharded stand-in over the same rows)"""
    from _helpers import STREAMS
    from _standin_shard_update import OneUpdateFeatureDB, ShardUpdateFeatureDB
    from video_query_algorithms_amd.shard import shard_range
    from video_query_algorithms_amd.sharded_db import ShardedFeatureDB
    r0, cnt = shard_range(x.shape[0], dist.get_world_size(), dist.get_rank())
    kw = {"stream_names": list(STREAMS), "slot_splits": [[1, 2, 3]] * 2}
    local = ShardUpdateFeatureDB(x[r0:r0 + cnt], clip_ids=ids[r0:r0 + cnt], **kw)
    one = OneUpdateFeatureDB(x, clip_ids=ids, **kw)
    local.planted = one.planted = planted
    return ShardedFeatureDB(local, x.shape[0], r0, ids, served=served, batch_rounds=batch_rounds), one


def _pass(db, x, Q):
    import sim_oracle as so
    refs = [(5 * q + 3) % N for q in range(Q)]
    t = np.stack([np.stack([[so.scale_feature(x[r, s, e].astype(np.float64)) for e in range(E)] for s in range(S)]) for r in refs])
    w = np.stack([[1.0, 0.5 + 0.125 * q] for q in range(Q)])
    return db.query_round_batch(t, w, np.array([[0.8, 0.6]] * Q))


def _group(one, world):
    """Five entries, not in query order, on the last round of ``one`` (5 queries) -> the arguments of batch_round_update.
    q 3: revise; its labelled rows lie on every shard, either side of every shard boundary, row 0 twice; one of them is planted -0.0.
    q 0: no labels (skipped), between served entries.
    q 4: finalize; every user row on the LAST rank; one labelled row is planted NaN (its whole surface is NaN: the pick is cell 0, 0).
    q 1: finalize without user rows (lowest 1.0).
    q 2: finalize; user rows on every shard, one of them planted -0.0; labels that put the minimum inside the grid."""
    import video_query_algorithms_amd as vqa
    from _pick_cases import candidates, compute_eps, make_hp
    from video_query_algorithms_amd.shard import shard_range
    hp = make_hp(vqa)
    edges = [shard_range(N, world, g)[0] for g in range(1, world)]
    last0 = edges[-1]
    rng = np.random.default_rng(world)
    members = [3, 0, 4, 1, 2]
    near_boundaries = [r for e in edges for r in (e, e - 1)]
    rows = [np.array(near_boundaries + [N - 1, 0, N // 2, 0] + list(rng.integers(0, N, size=9))), np.zeros(0, dtype=np.int64),
            np.array([1, last0, 7, edges[0], N - 2] + list(rng.integers(0, N, size=6))), np.array([5, edges[0] - 1, N - 1, 5]), None]
    users = [[], [], sorted({last0, last0 + 2, N - 1}), [], sorted({0, edges[0] - 1, edges[0], N - 1, 9})]
    labels = [(rng.random(r.size) < 0.4).astype(np.float64) if r is not None else None for r in rows]
    # q 2: the 24 best clips under weight 1.3, the better half confirmed, some verdicts flipped (tests/_standin_update.labelled_inside)
    import sim_oracle as so
    v = so.dense_scores(one._kept[2][0], [1.0, 1.3])
    best = np.argsort(-v)[:24]
    rows[4] = best
    labels[4] = np.array([float(bool(v[r] >= v[best[12]]) ^ bool(rng.random() < 0.12)) for r in best])
    finalize = [False, False, True, True, True]
    k = len(members)
    return (members, rows, labels, [candidates(hp)] * k, [hp.threshold_grid] * k, [hp.ballast] * k, [1] * k, compute_eps(),
            [None if f else hp.near_miss_default for f in finalize], users)


def _planted(ids, world):
    from video_query_algorithms_amd.shard import shard_range
    edge = shard_range(N, world, 1)[0]
    return {(3, int(ids[edge])): [-0.0, 0.25], (4, int(ids[1])): [SNAN, 0.5], (2, int(ids[N - 1])): [0.375, -0.0]}


def _served_only(args):
    keep = [i for i, r in enumerate(args[1]) if len(r)]
    return keep, tuple([a[i] for i in keep] if isinstance(a, list) else a for a in args)


class _Counts:
    """Counts what one call of the sharded database announces and all-reduces (the payload all-reduce: ``_sum``; the error agreement
    of a served database is not data)."""

    def __init__(self, sdb):
        self.sdb, self.ops, self.sums = sdb, [], 0

    def __enter__(self):
        sdb, real_announce, real_sum = self.sdb, self.sdb._announce, self.sdb._sum

        def announce(op, *a, **kw):
            self.ops.append(op)
            return real_announce(op, *a, **kw)

        def total(arr):
            self.sums += 1
            self.dtype = np.asarray(arr).dtype
            return real_sum(arr)
        sdb._announce, sdb._sum = announce, total
        return self

    def __exit__(self, *exc):
        del self.sdb._announce, self.sdb._sum


def _check_update(sdb, one, x, check_tables=True):
    """batch_round_update on the sharded database == on the unsharded one, what moves between the ranks, and the ranking behind it."""
    from _search_set_cases import np_topk
    from video_query_algorithms_amd.hyperparameter import raw_loss_surface
    from video_query_algorithms_amd.sharded_db import OP_BATCH_UPDATE
    import sim_oracle as so
    world = sdb.world
    _pass(one, x, 5)
    _pass(sdb, x, 5)
    args = _group(one, world)
    members, rows, labels, users = args[0], args[1], args[2], args[9]
    keep, served_args = _served_only(args)
    want = dict(zip(keep, one.batch_round_update(*served_args)))
    sdb.local.log.clear()
    with _Gathers() as g, _Counts(sdb) as c:
        got = sdb.batch_round_update(*args, want_surface=True)
    # one announcement, one all-reduce (of integers), one N-sized gather of [n, served entries] scores, two small gathers
    assert c.ops == [OP_BATCH_UPDATE] and c.sums == 1 and c.dtype == np.int64
    assert [call[1:] for call in g.calls] == [(N, len(keep)), (world, 4 * len(keep)), (world, g.calls[2][2])] and g.calls[0][0] == sdb.local.n
    assert [kind for kind, _ in sdb.local.log] == ["avg_rows", "update_given"]
    if check_tables:                                                      # every rank was handed the unsharded rows' values, bit for bit
        label_avgs, user_avgs = sdb.local.given
        for i, q in enumerate(members):
            assert _bits(label_avgs[i], one._kept[q][0][rows[i]]), ("labelled", q)
            assert _bits(user_avgs[i], one._kept[q][0][np.asarray(users[i], dtype=np.int64)]), ("user", q)
        assert np.signbit(label_avgs[0]).any() and np.signbit(user_avgs[4]).any() and _bits(label_avgs[2][0, 0], SNAN)
    assert len(got) == len(members)
    for i, q in enumerate(members):
        a = got[i]
        assert _bits(a.avg, one._kept[q][0]) and _same(a.n_e, one._kept[q][1])
        if i not in want:                                                 # the skipped entry: as the round left it, nothing picked
            assert all(getattr(a, f) is None for f in ("scores", "match_rows", "near_rows", "surface", "w", "threshold", "lowest", "band", "iw", "it",
                                                       "on_rim", "fell_back")) and a.near_argmax == -1
            continue
        b = want[i]
        assert _bits(a.w, b.w) and _bits(a.threshold, b.threshold) and _bits(a.lowest, b.lowest) and _bits(a.band, b.band), q
        assert (a.iw, a.it, a.on_rim, a.fell_back) == (b.iw, b.it, b.on_rim, b.fell_back), q
        assert _bits(a.scores, b.scores) and _same(a.match_rows, b.match_rows) and _same(a.near_rows, b.near_rows) and a.near_argmax == b.near_argmax, q
        graded = np.stack([so.dense_scores(one._kept[q][0][rows[i]], w) for w in args[3][i]])
        assert _bits(a.surface, raw_loss_surface(graded, labels[i], args[4][i], args[5][i])), q
    by_q = {q: want[i] for i, q in enumerate(members) if i in want}
    assert by_q[1].lowest == 1.0 and by_q[4].lowest < 1.0 and by_q[2].lowest < 1.0          # no user rows | rows on the last rank | on every rank
    assert not by_q[2].on_rim and (by_q[4].iw, by_q[4].it) == (0, 0) and np.isnan(by_q[4].scores).sum() == 1
    assert all(len(b.match_rows) + len(b.near_rows) > 0 for q, b in by_q.items() if q != 4)
    # the ranking behind the update stands under the updated scores
    qs = [members[i] for i in keep]
    ks = [3 + 5 * j for j in range(len(qs))]
    for (r_a, v_a), (r_b, v_b), q in zip(sdb.batch_round_topk(ks, qs), one.batch_round_topk(ks, qs), qs):
        assert _same(r_a, r_b) and _bits(v_a, v_b) and _same(r_b, np_topk(by_q[q].scores, len(r_b))[0]), q
    # ---- want_scores=False: nothing N-sized moves; the near maxima come from one grid call per rank; the ranking still follows
    _pass(sdb, x, 5)
    sdb.local.log.clear()
    with _Gathers() as g, _Counts(sdb) as c:
        lean = sdb.batch_round_update(*args, want_scores=False)
    assert c.ops == [OP_BATCH_UPDATE] and c.sums == 1
    assert len(g.calls) == 2 and all(call[1] == world and call[0] == 1 for call in g.calls)
    assert [kind for kind, _ in sdb.local.log if kind == "grid"] in ([], ["grid"])
    for i, q in enumerate(members):
        if i not in want:
            continue
        a, b = lean[i], want[i]
        assert a.scores is None and a.surface is None and _bits(a.w, b.w) and _bits(a.band, b.band) and _bits(a.lowest, b.lowest)
        assert _same(a.match_rows, b.match_rows) and _same(a.near_rows, b.near_rows) and a.near_argmax == b.near_argmax, q
    for (r_a, v_a), (r_b, v_b) in zip(sdb.batch_round_topk(ks, qs), one.batch_round_topk(ks, qs)):
        assert _same(r_a, r_b) and _bits(v_a, v_b)
    # every entry without labels: nothing is announced
    with _Counts(sdb) as c:
        none = sdb.batch_round_update([1, 0], [[], []], [[], []], args[3][:2], args[4][:2], [0.3, 0.3], [1, 1], args[7], [0.5, None], [[], [3]])
    assert not c.ops and not c.sums and all(r.w is None and r.scores is None for r in none)


def _check_refusals(sdb, x):
    """What is refused before anything is announced: the next call finds every rank in step."""
    from video_query_algorithms_amd import VqError
    args = list(_group_plain())
    with _Counts(sdb) as c:
        with pytest.raises(VqError) as ei:                                # a query the round did not have
            sdb.batch_round_update([16] + args[0][1:], *args[1:])
        assert ei.value.code == -4
        bad = [np.array([N])] + args[1][1:]
        with pytest.raises(ValueError):                                   # a labelled row outside the database
            sdb.batch_round_update(args[0], bad, *args[2:])
        with pytest.raises(ValueError):                                   # a user row outside the database
            sdb.batch_round_update(*args[:9], [[-1]] + args[9][1:])
        with pytest.raises(ValueError):                                   # one argument too short
            sdb.batch_round_update(*args[:5], args[5][:-1], *args[6:])
        with pytest.raises(ValueError):                                   # a column the grids do not have
            sdb.batch_round_update(*args[:6], [S] * len(args[0]), *args[7:])
        sdb.define_search_set("few", sdb.clip_ids[:5])
        sdb.use_search_set("few")
    ops_before = list(c.ops)
    with _Counts(sdb) as c:
        with pytest.raises(ValueError, match="search set"):
            sdb.batch_round_update(*args)
    assert not c.ops and not c.sums
    sdb.use_search_set(None)
    from video_query_algorithms_amd.sharded_db import OP_BATCH_UPDATE
    assert OP_BATCH_UPDATE == 24 and OP_BATCH_UPDATE not in ops_before


def _group_plain():
    """A small valid group for the refusals: two revise entries on queries 0 and 1."""
    import video_query_algorithms_amd as vqa
    from _pick_cases import candidates, compute_eps, make_hp
    hp = make_hp(vqa)
    return ([0, 1], [np.array([3, 40, 9]), np.array([50, 2])], [np.array([1.0, 0.0, 1.0]), np.array([0.0, 1.0])], [candidates(hp)] * 2,
            [hp.threshold_grid] * 2, [hp.ballast] * 2, [1, 1], compute_eps(), [0.5, 0.5], [[], []])


def _rows():
    import sim_oracle as so
    return so.synth_features(5, 0, N, S, E, D, (4.0, 1.0)), np.arange(100, 100 + N)


def _spmd_worker(rank, world, port, tmp):
    _setup(rank, world, port)
    from video_query_algorithms_amd import VqError
    x, ids = _rows()
    sdb, one = _databases(x, ids, served=False, planted=_planted(ids, world))
    with pytest.raises(VqError) as ei:                                    # no batched round yet (VQ_E_STATE, as on one GPU)
        sdb.batch_round_update(*_group_plain())
    assert ei.value.code == -4
    _check_update(sdb, one, x)
    _check_refusals(sdb, x)
    _check_update(sdb, one, x)                                            # the refusals left every rank in step
    off, _ = _databases(x, ids, served=False, batch_rounds=False)
    with pytest.raises(ValueError, match="batch_rounds"):
        off.batch_round_update(*_group_plain())
    np.save(os.path.join(tmp, "ok_%d.npy" % rank), np.zeros(1))
    sdb.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_spmd_sharded_update_equals_unsharded(tmp_path, world):
    mp.spawn(_spmd_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok_%d.npy" % r)) for r in range(world))


def _served_worker(rank, world, port, tmp):
    _setup(rank, world, port)
    from video_query_algorithms_amd.sharded_db import ShardError
    x, ids = _rows()
    sdb, one = _databases(x, ids, served=True, planted=_planted(ids, world))
    if rank == 0:
        _check_update(sdb, one, x)
        # rank 1's local update fails once: an exception on the broker, not a hang, and the next operation on the same database works
        args = list(_group_plain())
        args[3] = [np.array(g) for g in args[3]]
        args[3][0][:, 0] = 7.0
        with pytest.raises(ShardError, match=r"rank\(s\) \[1\]"):
            sdb.batch_round_update(*args)
        assert len(sdb.batch_round_topk(3)) == 5
        _check_refusals(sdb, x)
        _check_update(sdb, one, x)
        np.save(os.path.join(tmp, "ok.npy"), np.zeros(1))
        sdb.close()
    else:
        if rank == 1:
            sdb.local.fail_on = 7.0
        sdb.serve()                                                       # returns when rank 0 closes the database
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_served_sharded_update_equals_unsharded_and_survives_a_failing_rank(tmp_path, world):
    mp.spawn(_served_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    assert os.path.exists(tmp_path / "ok.npy")


# ---- the ticket seam: fit_on_device reaches the sharded database ------------------------------------------------------------------------
def _ticket_run(db, labelled):
    """Five tickets -- a revise, a finalize and a finalize without confirmed matches among them -- through
    compute_similarities_batch(fit=, fit_on_device=True, finalize=, top=) and their review sets."""
    import video_query_algorithms_amd as vqa
    from _helpers import DEFAULT_WEIGHTS, SEED
    from test_batch_tickets_standin import _hp, _ticket
    hp = _hp()
    (m60, u60), (m90, u90) = labelled[60], labelled[90]
    tickets = [_ticket(db, 60, hp, matches=m60, user_matches=u60), _ticket(db, 5, hp), _ticket(db, 90, hp, matches=m90, user_matches=u90),
               _ticket(db, 130, hp), _ticket(db, 150, hp, matches=m90, user_matches={})]
    finalize = [False, False, True, False, True]
    random.seed(a=SEED)
    vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, False, True, False, True], fit_on_device=True, finalize=finalize, top=[5, 7, 300, 1, 9])
    out = []
    for tk, fin in zip(tickets, finalize):
        weights, th = tk._fit if tk._fit is not None else (dict(DEFAULT_WEIGHTS), 0.8)
        tk.compute_scores(weights)
        budget, reach = (tk.number_of_matches_to_review, hp.near_miss_default)
        if fin:                                                           # compute_matches._review_budget; nobody confirmed: lowest stays 1.0
            lowest = tk.lowest_scoring_user_match()[0] if tk.user_matches else 1.0
            budget, reach = float("inf"), max(th - lowest, 0) / max(1 - th, float(os.environ["COMPUTE_EPS"]))
        tk.select_clips_to_review(th, budget, reach)
        out.append((tk._fit, dict(tk._ahead), tk._top, list(tk.matches.items())))
    return out, random.getstate()


def _same_ticket(got, want):
    (fit_a, ahead_a, top_a, matches_a), (fit_b, ahead_b, top_b, matches_b) = got, want
    assert fit_a == fit_b and matches_a == matches_b and len(matches_a) > 0
    assert ahead_a["w"] == ahead_b["w"] and ahead_a["select"] == ahead_b["select"] and ahead_a["near_argmax"] == ahead_b["near_argmax"]
    assert all(_same(ahead_a[k], ahead_b[k]) for k in ("scores", "match_rows", "near_rows"))
    assert _same(top_a[0], top_b[0]) and _same(top_a[1], top_b[1])


def _broker_run(db, labelled):
    """compute_matches(batch=True, fit_weights="device", top=4) over new, revise and finalize updates on ``db``."""
    import video_query_algorithms_amd as vqa
    from _helpers import SEED
    from test_batch_fit_standin import LATER, _outcome
    from test_batch_tickets_standin import _hp, _Repo, _update

    def again(row, kind):
        matches, user = labelled[row]
        return (kind, _update(row, feature_db=db, matches=matches, user_matches=user, **LATER))
    pairs = [("new", _update(5, feature_db=db)), again(60, "revise"), ("new", None), again(60, "finalize"), ("new", _update(130, feature_db=db)),
             again(90, "revise")]
    made, real_init = [], vqa.Ticket.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    vqa.Ticket.__init__ = spy
    hp = _hp()
    try:
        random.seed(a=SEED)
        vqa.compute_matches(_Repo(pairs), hp, batch=True, fit_weights="device", top=4)
    finally:
        vqa.Ticket.__init__ = real_init
    return _outcome(made, hp), [(tk._fit, tk._ahead["scores"], tk._top) for tk in made], random.getstate()


def _tickets_worker(rank, world, port, tmp):
    _setup(rank, world, port)
    from test_batch_tickets_standin import IDS, X, _db, _labelled
    from _standin_shard_update import OneUpdateFeatureDB
    on, one = _databases(X, IDS, served=True)
    if rank == 0:
        plain = _db(OneUpdateFeatureDB)
        labelled = {row: _labelled(plain, row) for row in (60, 90)}
        kinds = ("batch", "grid", "fit", "rescore", "update", "avg_rows", "update_given", "btopk", "scan", "select", "write_avg")
        want, want_state = _ticket_run(one, labelled)
        assert [kind for kind, _ in one.log if kind in kinds] == ["batch", "update", "btopk"]
        assert [w[0] is not None for w in want] == [True, False, True, False, True] and len(want[2][2][0]) == 300
        on.local.log.clear()
        got, got_state = _ticket_run(on, labelled)
        # the device mode reaches the sharded database: one pass, the rows' avg, the one local update, the ranking -- no grid, no rescore
        assert [kind for kind, _ in on.local.log if kind in kinds] == ["batch", "avg_rows", "update_given", "btopk"]
        for a, b in zip(got, want):
            _same_ticket(a, b)
        assert got_state == want_state                                    # `random` is left in the same state
        one.log.clear()
        on.local.log.clear()
        (want_out, want_tk, want_state), (got_out, got_tk, got_state) = _broker_run(one, labelled), _broker_run(on, labelled)
        assert got_out == want_out and got_state == want_state and [kind for kind, _ in one.log if kind in kinds] == ["batch", "update", "btopk"]
        assert [kind for kind, _ in on.local.log if kind in kinds] == ["batch", "avg_rows", "update_given", "btopk"]
        for (fit_a, scores_a, top_a), (fit_b, scores_b, top_b) in zip(got_tk, want_tk):
            assert fit_a == fit_b and _same(scores_a, scores_b) and _same(top_a[0], top_b[0]) and _same(top_a[1], top_b[1])
        assert sum(fit is not None for fit, _s, _t in want_tk) == 3
        np.save(os.path.join(tmp, "ok.npy"), np.zeros(1))
        on.close()
    else:
        on.serve()
    dist.destroy_process_group()


def test_fit_on_device_reaches_a_served_sharded_database(tmp_path):
    mp.spawn(_tickets_worker, args=(2, _port(), str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok.npy")
