"""Test program (GPU box): search sets on a served ShardedFeatureDB with the real kernels, against an ordinary one-GPU FeatureDB under
the same sets.  Started by tests/test_search_set_sharded_gpu.py as a process of its own (``ShardedFeatureDB.open`` starts the worker
ranks): every rank on the box's ONE card over gloo, or ONE rank over RCCL.  Prints ``ok``; any difference is an assertion."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("COMPUTE_EPS", "0.000003")


def main():
    world, backend = int(sys.argv[1]), sys.argv[2]
    import video_query_algorithms_amd as vqa
    from video_query_algorithms_amd.feature_store import save_store
    from video_query_algorithms_amd.shard import shard_range
    from video_query_algorithms_amd.sharded_db import ShardedFeatureDB
    from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS, golden_json, golden_npy, records_from_dense
    from _search_set_cases import check_two_tickets, host_loss_surface, np_min_score, np_select, np_topk, same_bits
    g = golden_json("real_subset.json")
    x = golden_npy("real_subset_x.npy")
    ids = np.asarray(g.get("clip_ids") or g["clip_order"], dtype=np.int64)
    n = x.shape[0]
    recs = records_from_dense(x, ids, [1, 2, 3])
    with tempfile.TemporaryDirectory() as d:
        store = save_store(os.path.join(d, "store"), x, ids, STREAMS, [1, 2, 3])
        sdb = ShardedFeatureDB.open(store, gpus=[0] * world, backend=backend)      # before this process's first GPU call
        try:
            one = vqa.FeatureDB.from_store(store)
            # ---- everything behind the scan, under views: one that leaves a rank without rows, an empty one, one clip, all
            r1, n1 = shard_range(n, world, min(1, world - 1))
            sets = {"skip": np.array([r for r in range(n) if (world == 1 or not r1 <= r < r1 + n1) and r % 4 != 2]),
                    "none": np.zeros(0, np.int64), "last": np.array([n - 1]), "all": np.arange(n)}
            t = one.set_query_from_row(2)
            assert same_bits(sdb.set_query_from_row(2), t)                          # database rows, view or no view
            w = np.array([1.0, 1.5])
            wg = np.stack([np.ones(40), np.arange(0.5, 2.5, 0.05)], 1)
            th_grid = np.arange(0.5, 1.1, 0.02)
            for name, rows in sets.items():
                for db in (one, sdb):
                    assert (db.define_search_set(name, ids[rows][::-1]).rows == rows).all()
            for name in ["skip", "none", None, "last", "all", "skip"]:
                m = n if name is None else sets[name].size
                for db in (one, sdb):
                    assert db.use_search_set(name).n == m
                    db.set_query(t)
                    db.scan(weights=w, keep_sims=True)
                a, b = one.similarities(sims=True), sdb.similarities(sims=True)
                assert all(same_bits(p, q) for p, q in zip(a, b)) and b[0].shape == (m, 2), name
                sc = one.scores()
                assert same_bits(sdb.scores(), sc)
                fin = np.sort(sc)
                th = float(fin[-max(1, m // 4)]) if m else 0.5
                want = np_select(sc, th, th - 0.2)
                for db in (one, sdb):
                    got = db.select(th, th - 0.2)
                    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2] == want[2], name
                    rk, vk = db.topk(7)
                    ok = np_topk(sc, 7)
                    assert (rk == ok[0]).all() and same_bits(np.ascontiguousarray(vk), ok[1]), name
                    pick = np.array([m - 1, 0, m // 2]) if m else np.zeros(0, np.int64)
                    assert db.min_score(pick) == np_min_score(sc, pick)
                if m:
                    ga, gb = one.scores_grid(wg, pick), sdb.scores_grid(wg, pick)
                    assert same_bits(ga, gb)
                    assert same_bits(one.loss_surface(wg, pick, [1.0, 0.0, 1.0], th_grid, 0.3), host_loss_surface(gb, [1.0, 0.0, 1.0], th_grid, 0.3))
                ra = one.query_round(t, weights=w, select=(th, th - 0.2))
                rb = sdb.query_round(t, weights=w, select=(th, th - 0.2))
                assert same_bits(ra.avg, rb.avg) and same_bits(np.ascontiguousarray(ra.n_e), rb.n_e) and same_bits(ra.scores, rb.scores)
                assert (ra.match_rows == rb.match_rows).all() and (ra.near_rows == rb.near_rows).all() and ra.near_argmax == rb.near_argmax
                rb2 = sdb.query_round(None, weights=[1.0, 0.7], select=(th, th - 0.2))
                ra2 = one.query_round(None, weights=[1.0, 0.7], select=(th, th - 0.2))
                assert same_bits(ra2.scores, rb2.scores) and (ra2.match_rows == rb2.match_rows).all() and ra2.near_argmax == rb2.near_argmax
                avg = np.ascontiguousarray(a[0][::-1])
                for db in (one, sdb):
                    db.write_avg(avg, np.ascontiguousarray(a[1][::-1]))
                    db.rescore(w)
                assert same_bits(one.scores(), sdb.scores())
            for db in (one, sdb):
                db.use_search_set(None)
                for name in sets:
                    db.drop_search_set(name)
            # ---- two tickets, two search sets, ONE served database (tests/_search_set_cases.py)
            check_two_tickets(vqa, sdb, lambda rows: vqa.FeatureDB.from_arrays(x[rows], clip_ids=ids[rows]), recs, x, ids, g, STREAMS,
                              DEFAULT_WEIGHTS, SEED)
            one.close()
        finally:
            sdb.close()
        assert all(p.returncode == 0 for p in sdb._workers), [p.returncode for p in sdb._workers]
    print("ok", flush=True)


if __name__ == "__main__":
    main()
