"""CPU, 2-3 processes over gloo: search sets on the row-sharded database (sharded_db.ShardedFeatureDB).

Every rank's "kernels" are the numpy stand-in with search sets (tests/_standin_views.py); under test is what ShardedFeatureDB adds:
the one announcement of a set as its ascending global rows, every rank's own sub-list, ``use`` as one announcement, gathers with
per-rank counts derived from the list (ragged shards, a rank with no row of the set, an empty set), positions in global view order.
Results must equal the UNSHARDED stand-in restricted to the same rows, exactly.  The GPU twin is tests/test_search_set_sharded_gpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _sharded(x, present, ids, served):
    from _helpers import STREAMS
    from _standin_views import ViewOracleFeatureDB
    from video_query_algorithms_amd.shard import shard_range
    from video_query_algorithms_amd.sharded_db import ShardedFeatureDB
    rank, world = dist.get_rank(), dist.get_world_size()
    r0, cnt = shard_range(x.shape[0], world, rank)
    local = ViewOracleFeatureDB(x[r0:r0 + cnt], None if present is None else present[r0:r0 + cnt], list(STREAMS), [[1, 2, 3]] * 2)
    return ShardedFeatureDB(local, x.shape[0], r0, ids, served=served)


def _spmd_worker(rank, world, port, n_total, tmp):
    _setup(rank, world, port)
    import sim_oracle as so
    from _search_set_cases import np_min_score, np_select, np_topk, presence_mask, same_bits
    from _standin_views import ViewOracleFeatureDB
    from video_query_algorithms_amd.shard import shard_range
    s, e, d = 2, 3, 64
    x = so.synth_features(5, 0, n_total, s, e, d, (4.0, 1.0))
    x[n_total // 2:] = x[:n_total - n_total // 2]                      # duplicated clips: exact score ties across shards and inside a view
    ids = np.arange(100, 100 + n_total)
    present = presence_mask(n_total, s, e)
    sdb = _sharded(x, present, ids, served=False)
    one = ViewOracleFeatureDB(x, present, clip_ids=ids)                 # the unsharded stand-in
    t = np.stack([[so.scale_feature(x[2, si, ei].astype(np.float64)) for ei in range(e)] for si in range(s)])
    r1, n1 = shard_range(n_total, world, 1)
    rng = np.random.default_rng(3)
    sets = {"half": np.sort(rng.choice(n_total, n_total // 2, replace=False)),
            "skip_rank_1": np.array([r for r in range(n_total) if not r1 <= r < r1 + n1 and r % 3 != 1]),   # rank 1 gets an empty sub-list
            "none": np.zeros(0, np.int64), "all": np.arange(n_total), "one": np.array([n_total - 1])}
    for name, rows in sets.items():
        clip_ids = ids[rows][::-1]                                     # any order
        v = sdb.define_search_set(name, clip_ids)
        w = one.define_search_set(name, clip_ids)
        assert (v.rows == rows).all() and (v.clip_ids == w.clip_ids).all() and v.n == rows.size
    with pytest.raises(KeyError):
        sdb.define_search_set("bad", [99])
    with pytest.raises(ValueError):
        sdb.define_search_set("half", [100])
    wg = np.stack([np.ones(5), np.linspace(0.5, 2.5, 5)], 1)
    for name in ["half", "skip_rank_1", None, "none", "all", "one", "half"]:
        rows = np.arange(n_total) if name is None else sets[name]
        m = rows.size
        view = sdb.use_search_set(name)
        one.use_search_set(name)
        assert view.n == m and sdb.use_search_set(name) is view
        assert sdb.local.use_search_set(sdb.local._in_use).n == np.count_nonzero((rows >= sdb.row0) & (rows < sdb.row0 + sdb.local.n))
        for db in (sdb, one):
            db.set_query(t)
            db.scan(weights=[1.0, 1.5], keep_sims=True)
        got, want = sdb.similarities(sims=True), one.similarities(sims=True)
        assert all(same_bits(a, b) for a, b in zip(got, want)) and got[0].shape == (m, s)
        sc = sdb.scores()
        assert same_bits(sc, one.scores()) and sc.shape == (m,)
        o_sims, o_avg, o_ne = so.dense_similarities(x[rows], t, present[rows])
        assert same_bits(got[0], o_avg) and same_bits(got[2], o_sims) and same_bits(sc, so.dense_scores(o_avg, [1.0, 1.5]))
        fin = np.sort(sc[~np.isnan(sc)])
        th = float(fin[-max(1, fin.size // 4)]) if fin.size else 0.5
        sel = sdb.select(th, th - 0.2)
        want_sel = np_select(sc, th, th - 0.2)
        assert (sel[0] == want_sel[0]).all() and (sel[1] == want_sel[1]).all() and sel[2] == want_sel[2]
        rows_k, vals_k = sdb.topk(9)
        o_rows, o_vals = np_topk(sc, 9)
        assert (rows_k == o_rows).all() and same_bits(vals_k, o_vals)
        pick = np.array([m - 1, 0, m // 2, min(3, m - 1)]) if m else np.zeros(0, np.int64)
        assert sdb.min_score(pick) == np_min_score(sc, pick)
        if m:
            assert same_bits(sdb.scores_grid(wg, pick), np.stack([so.dense_scores(o_avg[pick], w) for w in wg]))
            with pytest.raises(ValueError):
                sdb.min_score([m])                                    # a position outside the view
        # the round as one operation, with the scan and as a re-weighting
        r = sdb.query_round(t, weights=[1.0, 1.5], select=(th, th - 0.2))
        assert same_bits(r.avg, o_avg) and (r.n_e == o_ne).all() and r.n_e.dtype == np.int32 and same_bits(r.scores, sc)
        assert (r.match_rows == want_sel[0]).all() and (r.near_rows == want_sel[1]).all() and r.near_argmax == want_sel[2]
        r2 = sdb.query_round(None, weights=[1.0, 0.7], select=(th, th - 0.2))
        sc2 = so.dense_scores(o_avg, [1.0, 0.7])
        w2 = np_select(sc2, th, th - 0.2)
        assert r2.avg is None and same_bits(r2.scores, sc2) and (r2.match_rows == w2[0]).all() and (r2.near_rows == w2[1]).all() and r2.near_argmax == w2[2]
        # averaged similarities written back (a ticket's hand-back): [M, S], every rank takes its own positions
        sdb.write_avg(o_avg[::-1].copy(), o_ne[::-1].copy())
        sdb.rescore([1.0, 1.5])
        assert same_bits(sdb.scores(), so.dense_scores(o_avg[::-1], [1.0, 1.5]))
        with pytest.raises(ValueError):
            sdb.write_avg(np.zeros((m + 1, s)))
        # database rows stay database rows
        assert (sdb.read_rows([n_total - 1, 0]) == x[[n_total - 1, 0]]).all()
        if name is not None:
            with pytest.raises(Exception):
                sdb.scan_batch(t[None], np.array([[1.0, 1.5]]))
    with pytest.raises(ValueError):
        sdb.drop_search_set("half")                                   # in use
    sdb.use_search_set(None)
    sdb.drop_search_set("half")
    assert not sdb.has_search_set("half") and sdb.has_search_set("all")
    assert sdb.scan_batch(t[None], np.array([[1.0, 1.5]])).shape == (1, n_total)
    np.save(os.path.join(tmp, "ok_%d.npy" % rank), np.zeros(1))
    sdb.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_total,world", [(64, 2), (37, 3)])
def test_spmd_search_sets_equal_the_unsharded_stand_in(tmp_path, n_total, world):
    mp.spawn(_spmd_worker, args=(world, _port(), n_total, str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok_%d.npy" % r)) for r in range(world))


def _served_worker(rank, world, port):
    _setup(rank, world, port)
    import video_query_algorithms_amd as vqa
    from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS, golden_json, golden_npy, records_from_dense
    from _search_set_cases import check_two_tickets
    from _standin_views import ViewOracleFeatureDB
    from video_query_algorithms_amd.sharded_db import OP_DEFINE_SET, OP_USE_SET
    g = golden_json("real_subset.json")
    x = golden_npy("real_subset_x.npy")
    ids = np.asarray(g.get("clip_ids") or g["clip_order"], dtype=np.int64)
    sdb = _sharded(x, None, ids, served=True)
    try:
        if rank == 0:
            announced = []
            real_announce = type(sdb)._announce

            def counting(self, op, ints=(), floats=()):
                announced.append(op)
                return real_announce(self, op, ints, floats)
            type(sdb)._announce = counting
            try:
                check_two_tickets(vqa, sdb, lambda rows: ViewOracleFeatureDB(x[rows], clip_ids=ids[rows]),
                                  records_from_dense(x, ids, [1, 2, 3]), x, ids, g, STREAMS, DEFAULT_WEIGHTS, SEED)
            finally:
                type(sdb)._announce = real_announce
            assert announced.count(OP_DEFINE_SET) == 2                 # each set travels once
            assert 8 <= announced.count(OP_USE_SET) <= 40              # a switch per hand-back, none when the set does not change
            sdb.close()
        else:
            sdb.serve()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_two_tickets_on_a_served_sharded_database(world):
    mp.spawn(_served_worker, args=(world, _port()), nprocs=world, join=True)
