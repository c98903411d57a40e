"""CPU, 2-3 processes over gloo: the four calls of a batched round on a row-sharded database (ShardedFeatureDB(batch_rounds=True):
query_round_batch, batch_round_fit, batch_round_rescore, batch_round_topk) against the same calls on the unsharded database.

Every rank's "kernels" are the numpy stand-in of tests/_standin_shard_rounds.py, so under test is what ShardedFeatureDB adds: the
announcements, the one packed gather of the per-row results, the two small gathers that merge all partitions, the exact all-reduce
of the grid scores and the label-order sum behind it, the top-k merge, the error agreement -- and ticket.compute_similarities_batch
on top of them, unchanged.  Everything is compared with ==.  The GPU twin is tests/test_batch_sharded_gpu.py."""
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, E, D = 2, 3, 64


def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _setup(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("COMPUTE_EPS", "0.000003")
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _databases(x, ids, served, batch_rounds=True):
    """(the sharded database of this rank, the unsharded stand-in over the same rows)"""
    from _helpers import STREAMS
    from _standin_shard_rounds import ShardRoundsFeatureDB
    from video_query_algorithms_amd.shard import shard_range
    from video_query_algorithms_amd.sharded_db import ShardedFeatureDB
    r0, cnt = shard_range(x.shape[0], dist.get_world_size(), dist.get_rank())
    kw = {"stream_names": list(STREAMS), "slot_splits": [[1, 2, 3]] * 2}
    local = ShardRoundsFeatureDB(x[r0:r0 + cnt], clip_ids=ids[r0:r0 + cnt], **kw)
    return ShardedFeatureDB(local, x.shape[0], r0, ids, served=served, batch_rounds=batch_rounds), ShardRoundsFeatureDB(x, clip_ids=ids, **kw)


def _tied_rows(n_total):
    """Features whose second half repeats the first: every score has an exact twin on another shard (rows r and r + n // 2)."""
    import sim_oracle as so
    x = so.synth_features(5, 0, n_total, S, E, D, (4.0, 1.0))
    x[n_total // 2:] = x[: n_total - n_total // 2]
    return x


class _Gathers:
    """Counts the all_gather_rows calls of sharded_db and records (rows of this rank's part, rows of the result, columns)."""

    def __enter__(self):
        from video_query_algorithms_amd import sharded_db
        self.mod, self.real, self.calls = sharded_db, sharded_db.all_gather_rows, []

        def counting(local, n_total, group=None):
            self.calls.append((int(local.shape[0]), int(n_total), int(np.prod(local.shape[1:]))))
            return self.real(local, n_total, group)
        sharded_db.all_gather_rows = counting
        return self

    def __exit__(self, *exc):
        self.mod.all_gather_rows = self.real


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def _same_result(got, want, avg=True, scores=True, select=True):
    assert (got.avg is None) == (not avg) and (got.scores is None) == (not scores)
    if avg:
        assert _same(got.avg, want.avg) and _same(got.n_e, want.n_e) and got.n_e.dtype == np.int32
    if scores:
        assert _same(got.scores, want.scores)
    if select:
        assert _same(got.match_rows, want.match_rows) and _same(got.near_rows, want.near_rows) and got.near_argmax == want.near_argmax
    else:
        assert got.match_rows is None and got.near_rows is None and got.near_argmax == -1


def _check_rounds(sdb, one, x, Q):
    """The four calls with Q queries on the tied rows: sharded == unsharded, the tie rules, and what moves between the ranks."""
    import sim_oracle as so
    from _search_set_cases import np_topk
    from video_query_algorithms_amd.shard import shard_range
    n, world = x.shape[0], sdb.world
    edge = shard_range(n, world, 1)[0]
    refs = [(5 * q + 3) % n for q in range(Q)]
    t = np.stack([np.stack([[so.scale_feature(x[r, s, e].astype(np.float64)) for e in range(E)] for s in range(S)]) for r in refs])
    w = np.stack([[1.0, 0.5 + 0.125 * q] for q in range(Q)])
    plain = one.query_round_batch(t, w)
    ths = [float(np.sort(r.scores)[-(n // 4)]) for r in plain]
    bands = np.array([[th, th - 0.2] for th in ths])
    want = one.query_round_batch(t, w, bands)
    # ---- the pass: one gather of [n_local, Q S + S + Q] into N rows, two small ones for all Q partitions
    with _Gathers() as g:
        got = sdb.query_round_batch(t, w, bands)
    assert [c[1:] for c in g.calls] == [(n, Q * S + S + Q), (world, 4 * Q), (world, g.calls[2][2])] and g.calls[0][0] == sdb.local.n
    for a, b in zip(got, want):
        _same_result(a, b)
    assert all(r.n_e is got[0].n_e for r in got)                                     # one array shared by all results
    tied = 0
    for q, r in enumerate(want):                                                      # the near arg-max of a tied pair: its lower row
        if r.near_argmax >= 0:
            twins = np.flatnonzero(r.scores == r.scores[r.near_argmax])
            tied += twins.size > 1
            assert r.near_argmax == twins[0] and got[q].near_argmax == twins[0]
    assert tied, "no query's near band has its maximum on a tied pair: the tie rule is not exercised"
    with _Gathers() as g:                                                             # without bands: the one gather alone
        for a, b in zip(sdb.query_round_batch(t, w), plain):
            _same_result(a, b, select=False)
    assert [c[1] for c in g.calls] == [n]
    # ---- nothing N-sized moves when neither avg nor scores are wanted; the near maxima come from one grid call per rank
    sdb.local.log.clear()
    with _Gathers() as g:
        lean = sdb.query_round_batch(t, w, bands, want_avg=False, want_scores=False)
    assert len(g.calls) == 2 and all(c[1] == world and c[0] == 1 for c in g.calls)
    mine = any(((r.near_rows >= sdb.row0) & (r.near_rows < sdb.row0 + sdb.local.n)).any() for r in want)
    assert [kind for kind, _ in sdb.local.log if kind == "grid"] == (["grid"] if mine else [])
    for a, b in zip(lean, want):
        _same_result(a, b, avg=False, scores=False)
    # ---- the ranking on the scores the lean pass left on the ranks: one gather; ties by ascending GLOBAL row
    ks = [(3 + 7 * q) % (n + 4) + 1 for q in range(Q)]
    with _Gathers() as g:
        ranked = sdb.batch_round_topk(ks)
    assert len(g.calls) == 1 and g.calls[0][1] == world
    for q, (rows, vals) in enumerate(ranked):
        o_rows, o_vals = np_topk(want[q].scores, ks[q])
        assert _same(rows, o_rows) and _same(vals, o_vals), q
        twins = [i for i in range(len(rows) - 1) if vals[i] == vals[i + 1]]
        assert all(rows[i] < rows[i + 1] for i in twins) and (twins or len(rows) < 2)
    assert _same(sdb.batch_round_topk(4, [Q - 1])[0][0], np_topk(want[Q - 1].scores, 4)[0])
    # ---- the fit: labelled rows on every shard, a repeated row, an entry without labels, entries not in query order
    rng = np.random.default_rng(Q)
    cand = np.stack([np.ones(40), np.arange(0.5, 2.5, 0.05)], axis=1)
    th_grid = np.arange(0.5, 1.1, 0.02)
    members = [[0], [1, 0], [Q - 1, 0, 1]][min(Q, 3) - 1]
    rows = [np.concatenate([[n - 1, 0, n // 2, 0], rng.integers(0, n, size=9)]), np.zeros(0, dtype=np.int64),
            np.array([edge, edge - 1, n - 1, 0, 7])][:len(members)]                  # the rows either side of the first shard boundary
    labels = [(rng.random(r.size) < 0.4).astype(np.float64) for r in rows]
    args = (members, rows, labels, [cand] * len(members), [th_grid] * len(members), [0.3] * len(members))
    one.query_round_batch(t, w, bands)
    with _Gathers() as g:
        surfaces = sdb.batch_round_fit(*args)
    assert not g.calls                                                                # an all-reduce, no gather
    for a, b, r in zip(surfaces, one.batch_round_fit(*args), rows):
        assert (a is None and r.size == 0) or (a.shape == (40, 31) and _same(a, b))
    # ---- the re-weighting, merged like the pass; the ranking then stands under the new scores
    new_w = np.stack([[1.0, 2.25 - 0.125 * i] for i in range(len(members))])
    new_bands = np.array([[ths[q] - 0.05, ths[q] - 0.3] for q in members])
    with _Gathers() as g:
        again = sdb.batch_round_rescore(members, new_w, new_bands)
    assert [c[1:] for c in g.calls] == [(n, len(members)), (world, 4 * len(members)), (world, g.calls[2][2])]
    o_again = one.batch_round_rescore(members, new_w, new_bands)
    for a, b, q in zip(again, o_again, members):
        assert _same(a.scores, b.scores) and _same(a.match_rows, b.match_rows) and _same(a.near_rows, b.near_rows) and a.near_argmax == b.near_argmax
        assert a.avg is None and a.n_e is None                                        # the round's own: the lean pass kept none
        rows_q, vals_q = sdb.batch_round_topk([6], [q])[0]
        assert _same(rows_q, np_topk(b.scores, 6)[0]) and _same(vals_q, np_topk(b.scores, 6)[1])
    sdb.query_round_batch(t, w, bands)
    for a, q in zip(sdb.batch_round_rescore(members, new_w), members):
        assert _same(a.avg, want[q].avg) and _same(a.n_e, want[q].n_e) and a.match_rows is None


def _check_refusals(sdb, x):
    """What is refused, before anything is announced: the next call finds every rank in step."""
    from video_query_algorithms_amd import VqError
    t, w = np.zeros((17, S, E, D)), np.ones((17, S))
    with pytest.raises(ValueError, match="1 to 16"):
        sdb.query_round_batch(t, w)
    with pytest.raises(ValueError):
        sdb.query_round_batch(t[:0], w[:0])
    with pytest.raises(NotImplementedError):
        sdb.query_round_batch(t[:2], w[:2], timed=True)
    with pytest.raises(ValueError):
        sdb.batch_round_fit([0], [[x.shape[0]]], [[1.0]], [np.ones((40, S))], [np.ones(31)], [0.3])       # a row outside the database
    with pytest.raises(VqError) as ei:
        sdb.batch_round_rescore([16], np.ones((1, S)))                                # a query the round did not have
    assert ei.value.code == -4
    with pytest.raises(VqError) as ei:
        sdb.batch_round_topk([1], [16])
    assert ei.value.code == -4
    from video_query_algorithms_amd import sharded_db
    cap, sharded_db.BATCH_TOPK_CAP = sharded_db.BATCH_TOPK_CAP, 8                     # the cap of a call, at a size these rows reach
    try:
        assert cap == 4096
        with pytest.raises(VqError) as ei:
            sdb.batch_round_topk(9)
        assert ei.value.code == -1
    finally:
        sharded_db.BATCH_TOPK_CAP = cap
    sdb.define_search_set("few", sdb.clip_ids[:5])
    sdb.use_search_set("few")
    for call in (lambda: sdb.query_round_batch(t[:2], w[:2]), lambda: sdb.batch_round_topk(3),
                 lambda: sdb.batch_round_rescore([0], np.ones((1, S)))):
        with pytest.raises(ValueError, match="search set"):
            call()
    sdb.use_search_set(None)


def _spmd_worker(rank, world, port, n_total, tmp):
    _setup(rank, world, port)
    from video_query_algorithms_amd import VqError
    x = _tied_rows(n_total)
    ids = np.arange(100, 100 + n_total)
    sdb, one = _databases(x, ids, served=False)
    assert sdb.batch_round_supported()
    with pytest.raises(VqError):                                                      # no batched round yet (VQ_E_STATE, as on one GPU)
        sdb.batch_round_topk(3)
    for Q in (1, 16):
        _check_rounds(sdb, one, x, Q)
    _check_refusals(sdb, x)
    _check_rounds(sdb, one, x, 3)                                                     # the refusals left every rank in step
    off, _ = _databases(x, ids, served=False, batch_rounds=False)
    assert not off.batch_round_supported()
    with pytest.raises(ValueError, match="batch_rounds"):
        off.query_round_batch(np.zeros((2, S, E, D)), np.ones((2, S)))
    np.save(os.path.join(tmp, "ok_%d.npy" % rank), np.zeros(1))
    sdb.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_total,world", [(64, 2), (37, 3)])
def test_spmd_batched_rounds_equal_unsharded(tmp_path, n_total, world):
    mp.spawn(_spmd_worker, args=(world, _port(), n_total, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok_%d.npy" % r)) for r in range(world))


def _served_worker(rank, world, port, n_total, tmp):
    _setup(rank, world, port)
    from video_query_algorithms_amd import VqError
    from video_query_algorithms_amd.sharded_db import ShardError
    x = _tied_rows(n_total)
    ids = np.arange(100, 100 + n_total)
    sdb, one = _databases(x, ids, served=True)
    if rank == 0:
        # rank 1's pass fails once: an exception on the broker, not a hang, and the next round on the same database works
        with pytest.raises(ShardError, match=r"rank\(s\) \[1\]"):
            sdb.query_round_batch(np.zeros((2, S, E, D)) + 1.0, np.full((2, S), 7.0))
        with pytest.raises(VqError):                                                  # the failed round left no snapshot to rank
            sdb.batch_round_topk(3)
        for Q in (16, 1):
            _check_rounds(sdb, one, x, Q)
        with pytest.raises(ShardError, match=r"rank\(s\) \[1\]"):                     # likewise in the re-weighting, behind a good round
            sdb.batch_round_rescore([0], np.full((1, S), 7.0))
        _check_refusals(sdb, x)
        _check_rounds(sdb, one, x, 2)
        np.save(os.path.join(tmp, "ok.npy"), np.zeros(1))
        sdb.close()
    else:
        if rank == 1:
            sdb.local.fail_on = 7.0
        sdb.serve()                                                                   # returns when rank 0 closes the database
    dist.destroy_process_group()


@pytest.mark.parametrize("n_total,world", [(64, 2), (37, 3)])
def test_served_batched_rounds_equal_unsharded_and_survive_a_failing_rank(tmp_path, n_total, world):
    mp.spawn(_served_worker, args=(world, _port(), n_total, str(tmp_path)), nprocs=world, join=True)
    assert os.path.exists(tmp_path / "ok.npy")


# ---- tickets: ticket.compute_similarities_batch, unchanged, on a served sharded database ---------------------------------------------
def _ticket_run(db, labelled):
    """Four tickets, two of them with verdicts, through compute_similarities_batch(fit=, top=) and their review sets."""
    import video_query_algorithms_amd as vqa
    from _helpers import DEFAULT_WEIGHTS, SEED
    from test_batch_tickets_standin import _hp, _ticket
    hp = _hp()
    tickets = [_ticket(db, 60, hp, matches=labelled[60][0], user_matches=labelled[60][1]), _ticket(db, 5, hp),
               _ticket(db, 90, hp, matches=labelled[90][0], user_matches=labelled[90][1]), _ticket(db, 130, hp)]
    random.seed(a=SEED)
    vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, False, True, False], top=[5, 7, 300, 1])
    out = []
    for tk in tickets:
        weights, th = tk._fit if tk._fit is not None else (dict(DEFAULT_WEIGHTS), 0.8)
        tk.compute_scores(weights)
        tk.select_clips_to_review(th, tk.number_of_matches_to_review, hp.near_miss_default)
        out.append((tk._fit, dict(tk._ahead), tk._top, list(tk.matches.items())))
    return out, random.getstate()


def _same_ticket(got, want):
    (fit_a, ahead_a, top_a, matches_a), (fit_b, ahead_b, top_b, matches_b) = got, want
    assert fit_a == fit_b and matches_a == matches_b and len(matches_a) > 0
    assert ahead_a["w"] == ahead_b["w"] and ahead_a["select"] == ahead_b["select"] and ahead_a["near_argmax"] == ahead_b["near_argmax"]
    assert all(_same(ahead_a[k], ahead_b[k]) for k in ("scores", "match_rows", "near_rows"))
    assert _same(top_a[0], top_b[0]) and _same(top_a[1], top_b[1])


def _tickets_worker(rank, world, port, tmp):
    _setup(rank, world, port)
    from test_batch_tickets_standin import IDS, X, _db, _labelled
    from _standin_shard_rounds import ShardRoundsFeatureDB
    on, one = _databases(X, IDS, served=True)
    off, _ = _databases(X, IDS, served=True, batch_rounds=False)
    if rank == 0:
        plain = _db(ShardRoundsFeatureDB)
        labelled = {row: _labelled(plain, row) for row in (60, 90)}
        want, want_state = _ticket_run(one, labelled)
        assert [kind for kind, _ in one.log if kind in ("batch", "fit", "rescore", "btopk", "scan")] == ["batch", "fit", "rescore", "btopk"]
        assert want[0][0] is not None and want[2][0] is not None and want[1][0] is None and len(want[2][2][0]) == 300
        on.local.log.clear()
        got, got_state = _ticket_run(on, labelled)
        assert [kind for kind, _ in on.local.log if kind in ("batch", "grid", "fit", "rescore", "btopk", "scan")] == ["batch", "grid", "rescore", "btopk"]
        for a, b in zip(got, want):
            _same_ticket(a, b)
        assert got_state == want_state                                                # `random` is left in the same state
        on.close()
        # the default: the tickets run their own rounds, as before the switch existed
        called = []
        real = type(off).query_round_batch
        type(off).query_round_batch = lambda self, *a, **k: called.append(1) or real(self, *a, **k)
        try:
            alone, alone_state = _ticket_run(off, labelled)
        finally:
            type(off).query_round_batch = real
        assert not called and not off.batch_round_supported()
        assert [kind for kind, _ in off.local.log if kind in ("batch", "grid", "btopk")] == [] and all(a[0] is None for a in alone)
        assert all(len(a[3]) > 0 and a[1] is not None for a in alone)
        np.save(os.path.join(tmp, "ok.npy"), np.zeros(1))
        off.close()
    else:
        on.serve()
        off.serve()
    dist.destroy_process_group()


def test_tickets_share_a_pass_on_a_served_sharded_database_only_when_asked(tmp_path):
    mp.spawn(_tickets_worker, args=(2, _port(), str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok.npy")
