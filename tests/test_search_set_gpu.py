"""GPU: search sets on a resident feature database -- row views from the scan kernels (csrc/vq_sim.hip) up to Ticket.

A clip's dot products, ensemble means and score under a view are the full scan's sequence of operations on the same handle, so every
scan test compares BITS: position i of the view against row rows[i] of the same handle's full scan.  What runs behind the scan
(selection, top-k, grids, the one-call round) is checked against numpy on the view's own scores, exactly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sim_oracle as so
from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS, golden_json, golden_npy, records_from_dense
from _search_set_cases import (host_loss_surface, np_min_score, np_select, np_topk, presence_mask, same_bits, same_values, view_lists)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIM_TOL = 1e-12
N1 = 2051                                                  # odd, several blocks of 4 waves, 129 tiles of 16 with a ragged last one


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def _full_scan(db, w):
    db.use_search_set(None)
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    return avg, n_e, sims, db.scores()


def _check_view(db, name, rows, full, w, oracle=None):
    """Scan over the view and compare with rows ``rows`` of the full scan ``full`` of the same handle (and with the oracle's dots)."""
    avg, n_e, sims, sc = full
    db.define_search_rows(name, rows)
    view = db.use_search_set(name)
    assert view.n == rows.size and (view.rows == rows).all()
    db.scan(weights=w, keep_sims=True)
    v_avg, v_ne, v_sims = db.similarities(sims=True)
    v_sc = db.scores()
    m = rows.size
    assert v_avg.shape == (m, db.S) and v_ne.shape == (m, db.S) and v_sims.shape == (m, db.S, db.E) and v_sc.shape == (m,)
    assert same_bits(v_avg, avg[rows]), name
    assert same_bits(v_ne, n_e[rows]), name
    assert same_bits(v_sims, sims[rows]), name
    assert same_bits(v_sc, sc[rows]), name
    assert same_values(v_sc, so.dense_scores(v_avg, w)), name                    # the device's own averages, scored by the oracle
    if oracle is not None and m:
        assert np.abs(v_sims - oracle[rows]).max() <= SIM_TOL, name
    db.use_search_set(None)
    db.drop_search_set(name)


# ---------------------------------------------------------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.float16])
@pytest.mark.parametrize("s,e,d", [(1, 1, 1024), (2, 3, 1024), (2, 5, 1024), (3, 2, 260)])
def test_view_scan_equals_the_full_scan_of_the_same_handle(vqa, dtype, s, e, d):
    scales = (4.0, 1.0, 2.0)[:s]
    db = vqa.FeatureDB.synthetic(N1, s, e, d, seed=17, scales=scales, dtype=dtype)
    x = so.synth_features(17, 0, N1, s, e, d, scales).astype(dtype)              # what the device generated (fp16: rounded once)
    assert (db.read_rows([0, N1 - 1]) == x[[0, N1 - 1]]).all()
    t = np.random.default_rng(17).standard_normal((s, e, d)) / d
    w = [1.0, 1.5, 0.7][:s]
    db.set_query(t)
    lists = view_lists(N1)
    for present in (None, presence_mask(N1, s, e)):
        db.set_present(present)
        full = _full_scan(db, w)
        o_sims, o_avg, o_ne = so.dense_similarities(x, t, present)
        assert np.abs(full[2] - o_sims).max() <= SIM_TOL and (full[1] == o_ne).all()
        if present is not None:
            assert np.isnan(full[0][1, 0]) and full[1][1, 0] == 0 and np.isnan(full[3][N1 - 1])      # a (clip, stream) with no split present
        for name, rows in lists.items():
            _check_view(db, name, rows, full, w, oracle=o_sims)
        # the identity list IS the full scan; and after the views the full scan still is what it was
        again = _full_scan(db, w)
        assert all(same_bits(a, b) for a, b in zip(again, full))
    db.close()


# ---------------------------------------------------------------------------------------------------------------- 2. grid stride
def test_waves_that_walk_several_positions(vqa):
    """9 000 clips x 2 x 3 fp32: the grid is capped at 3 072 waves, a view of ~7 000 rows gives every wave two or three positions."""
    n, s, e, d = 9000, 2, 3, 1024
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=31)
    rng = np.random.default_rng(31)
    db.set_query(rng.standard_normal((s, e, d)) / d)
    rows = np.flatnonzero(rng.random(n) < 7000 / n)
    assert rows.size > 2 * 3072
    for present in (None, presence_mask(n, s, e)):
        db.set_present(present)
        _check_view(db, "stride", rows, _full_scan(db, [1.0, 1.5]), [1.0, 1.5])
    db.close()


@pytest.mark.parametrize("lean", ["0", "1"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_both_instantiations_of_the_scan_kernel_under_a_view(gpu, lean, dtype):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_search_set_scan_child.py"), lean, dtype], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------------------- 3. tiled
def test_tiled_database_walks_the_touched_tiles(vqa):
    n, s, e, d = 56_003, 2, 3, 1024                        # 3 501 tiles, the last one holds 3 clips
    ntiles = (n + 15) // 16
    rng = np.random.default_rng(7)
    parts = []
    for tile in range(ntiles - 1):
        kind = tile % 3
        if kind == 0:
            parts.append([16 * tile + 5])                  # one clip of the tile
        elif kind == 1:
            parts.append(range(16 * tile, 16 * tile + 16))   # a full tile
        elif tile % 10:                                    # some clips; every tenth of these tiles is not touched at all
            parts.append(16 * tile + np.sort(rng.choice(16, int(rng.integers(1, 16)), replace=False)))
    parts.append(range(16 * (ntiles - 1), n))              # the ragged last tile, row N - 1 included
    rows = np.concatenate([np.asarray(list(p) if isinstance(p, range) else p, dtype=np.int64) for p in parts])
    touched = np.unique(rows >> 4).size
    assert touched > 3072 and touched < ntiles and rows[-1] == n - 1 and (np.diff(rows) > 0).all()
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=23)
    db.set_query(np.random.default_rng(23).standard_normal((s, e, d)) / d)
    w = [1.0, 1.5]
    present = presence_mask(n, s, e)
    db.set_present(present)
    rows_full = _full_scan(db, w)
    _check_view(db, "on_rows", rows, rows_full, w)
    db.define_search_rows("before", rows)                  # defined while row-major ...
    db.set_layout("tiled")
    assert db.layout == "tiled"
    tiled_full = _full_scan(db, w)
    assert np.nanmax(np.abs(tiled_full[2] - rows_full[2])) <= SIM_TOL and not same_bits(tiled_full[2], rows_full[2])
    db.define_search_rows("after", rows)                   # ... and afterwards
    got = {}
    for name in ("before", "after"):
        db.use_search_set(name)
        db.scan(weights=w, keep_sims=True)
        got[name] = db.similarities(sims=True) + (db.scores(),)
        for a, b in zip(got[name], (tiled_full[0], tiled_full[1], tiled_full[2], tiled_full[3])):
            assert same_bits(a, b[rows]), name             # the tiled handle's own full scan, bit for bit
        assert np.nanmax(np.abs(got[name][2] - rows_full[2][rows])) <= SIM_TOL        # and the row-major handle to rounding
        assert same_values(got[name][3], so.dense_scores(got[name][0], w))
    assert all(same_bits(a, b) for a, b in zip(got["before"], got["after"]))
    # small views on the tiled database: nothing, one clip of the first tile, the last clip of the ragged tile
    for name, r in (("empty", np.zeros(0, np.int64)), ("first", np.array([0])), ("last", np.array([n - 1])), ("two", np.array([15, 16]))):
        _check_view(db, name, r, tiled_full, w)
    db.set_layout("rows")                                  # and back: the row form of the same view
    db.use_search_set("before")
    db.scan(weights=w, keep_sims=True)
    assert same_bits(db.similarities(sims=True)[2], rows_full[2][rows])
    db.close()


# ---------------------------------------------------------------------------------------------------------------- 4. behind the scan
@pytest.fixture(scope="module")
def big_db(vqa):
    n, s, e, d = 40_000, 2, 1, 1024
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=41)
    db.set_query_from_row(12_345)
    yield db
    db.close()


@pytest.mark.parametrize("m", [300, 20_000])               # both sides of the one-workgroup limits of selection and top-k (16 384)
def test_everything_behind_the_scan_works_on_positions(vqa, big_db, m):
    db, n = big_db, big_db.n
    rng = np.random.default_rng(m)
    rows = np.sort(rng.choice(n, m, replace=False))
    name = "m%d" % m
    db.define_search_rows(name, rows)
    db.use_search_set(name)
    w = np.array([1.0, 1.5])
    db.scan(weights=w)
    avg, n_e = db.similarities()
    # write_avg round-trips M rows: ties (copied rows) and NaNs planted in the averaged similarities, then rescored
    avg = avg.copy()
    avg[m // 3:m // 3 + 40] = avg[5]
    avg[[7, m // 2, m - 1], 0] = np.nan
    db.write_avg(avg, n_e)
    back = db.similarities()
    assert same_bits(back[0], avg) and same_bits(back[1], n_e)
    db.rescore(w)
    sc = db.scores()
    assert sc.shape == (m,) and same_values(sc, so.dense_scores(avg, w)) and np.isnan(sc).sum() == 3
    fin = np.sort(sc[~np.isnan(sc)])
    for th in (float(fin[-min(m // 4, 3000)]), float(fin[-11])):                 # match lists longer and shorter than the 1 024-row prefix
        lower = th - 0.05
        want = np_select(sc, th, lower)
        got = db.select(th, lower)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2] == want[2]
        r = db.query_round(None, weights=w, select=(th, lower))
        assert r.avg is None and same_bits(r.scores, sc) and (r.match_rows == want[0]).all() and (r.near_rows == want[1]).all() and r.near_argmax == want[2]
    assert want[0].size < 1024 and (m == 300 or np_select(sc, float(fin[-3000]), 0.0)[0].size > 1024)
    for k in (1, 25, m):
        rk, vk = db.topk(k)
        ok_rows, ok_vals = np_topk(sc, k)
        assert (rk == ok_rows).all() and same_bits(vk, ok_vals)
    assert db.topk(m)[0].size == m - 3                                           # NaNs excluded
    pick = np.array([m - 1, 0, m // 3 + 2, 5, 1, m - 2])
    finite = pick[1:]
    assert db.min_score(finite) == np_min_score(sc, finite) and db.min_score([]) == 1.0
    assert same_bits(db.scores_at(pick), sc[pick])
    wg = np.stack([np.ones(40), np.arange(0.5, 2.5, 0.05)], 1)
    graded = db.scores_grid(wg, finite)
    assert same_bits(graded, np.stack([so.dense_scores(avg[finite], g) for g in wg]))
    labels = [True, False, True, True, False]
    th_grid = np.arange(0.5, 1.1, 0.02)
    assert same_bits(db.loss_surface(wg, finite, [float(v) for v in labels], th_grid, 0.3), host_loss_surface(graded, labels, th_grid, 0.3))
    for call in (lambda: db.scores_at([m]), lambda: db.min_score([m]), lambda: db.scores_grid(wg, [0, m]),
                 lambda: db.loss_surface(wg, [m], [1.0], th_grid, 0.3)):
        with pytest.raises(vqa.VqError):                                         # position M is outside the view, though row M exists
            call()
    # the one-call round with the scan: every piece equals the separate calls, bit for bit
    t = db.set_query_from_row(12_345)                                            # a DATABASE row, view or no view
    db.scan(weights=w)
    s_avg, s_ne = db.similarities()
    s_sc = db.scores()
    th = float(np.sort(s_sc)[-min(m // 4, 3000)])
    s_sel = db.select(th, th - 0.05)
    r = db.query_round(t, weights=w, select=(th, th - 0.05))
    assert same_bits(r.avg, s_avg) and same_bits(r.n_e, s_ne) and same_bits(r.scores, s_sc)
    assert (r.match_rows == s_sel[0]).all() and (r.near_rows == s_sel[1]).all() and r.near_argmax == s_sel[2]
    assert (r.match_rows.size > 1024) == (m > 300)
    # the 16-query pass knows no views
    with pytest.raises(vqa.VqError) as err:
        db.scan_batch(t[None], w[None])
    assert err.value.code == -5                                                  # VQ_E_UNSUPPORTED
    db.use_search_set(None)
    assert db.scan_batch(t[None], w[None]).shape == (1, n)
    db.drop_search_set(name)


def test_an_empty_search_set(vqa, big_db):
    db = big_db
    db.define_search_rows("nothing", [])
    v = db.use_search_set("nothing")
    assert v.n == 0
    db.scan(weights=[1.0, 1.5])
    assert db.similarities()[0].shape == (0, 2) and db.scores().shape == (0,)
    m, r, am = db.select(0.5, 0.1)
    assert m.size == 0 and r.size == 0 and am == -1
    assert db.topk(5)[0].size == 0 and db.min_score([]) == 1.0
    kk = C.c_int64(-7)
    buf = np.zeros(4)
    rows = np.zeros(4, np.int64)
    vqa._lib.call("vq_db_topk", db._h, 4, rows.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.byref(kk))
    assert kk.value == 0
    rr = db.query_round(np.zeros((2, 1, 1024)), weights=[1.0, 1.5], select=(0.5, 0.1))
    assert rr.avg.shape == (0, 2) and rr.scores.shape == (0,) and rr.match_rows.size == 0 and rr.near_rows.size == 0 and rr.near_argmax == -1
    db.use_search_set(None)
    db.drop_search_set("nothing")


# ---------------------------------------------------------------------------------------------------------------- 5. the C ABI
def test_argument_errors_through_the_c_abi(vqa):
    lib = vqa.load_library()
    db = vqa.FeatureDB.synthetic(100, 1, 1, 64, seed=1, scales=(1.0,))
    vid = C.c_int32(-9)

    def define(rows):
        r = np.asarray(rows, dtype=np.int64)
        return lib.vq_db_rows_define(db._h, r.ctypes.data_as(C.c_void_p), r.size, C.byref(vid)), lib.vq_last_error().decode()
    rc, msg = define([3, 9, 7])
    assert rc == -1 and "strictly ascending" in msg and "rows[2] = 7" in msg
    rc, msg = define([3, 9, 9, 12])
    assert rc == -1 and "duplicate" in msg and "rows[2] = 9" in msg
    rc, msg = define([3, 9, 100])
    assert rc == -1 and "rows[2] = 100 outside [0,100)" in msg
    rc, msg = define([-1, 9])
    assert rc == -1 and "rows[0] = -1 outside" in msg
    assert vid.value == -9                                                       # nothing was defined
    ids = []
    for k in range(17):                                                          # at least 16 views stay resident
        rc, msg = define(np.arange(k, 100, 17))
        assert rc == 0, msg
        ids.append(vid.value)
    assert len(set(ids)) == 17 and min(ids) >= 0
    view, m = C.c_int32(), C.c_int64()
    assert lib.vq_db_rows_active(db._h, C.byref(view), C.byref(m)) == 0 and (view.value, m.value) == (-1, 100)
    assert lib.vq_db_rows_use(db._h, ids[4]) == 0
    assert lib.vq_db_rows_active(db._h, C.byref(view), C.byref(m)) == 0 and (view.value, m.value) == (ids[4], len(range(4, 100, 17)))
    assert lib.vq_db_rows_drop(db._h, ids[4]) == -4 and "in use" in lib.vq_last_error().decode()          # VQ_E_STATE
    assert lib.vq_db_rows_drop(db._h, 99) == -1 and "no row view 99" in lib.vq_last_error().decode()
    assert lib.vq_db_rows_use(db._h, 99) == -1 and "no row view 99" in lib.vq_last_error().decode()
    assert lib.vq_db_rows_use(db._h, -2) == -1
    assert lib.vq_db_rows_drop(db._h, ids[5]) == 0
    assert lib.vq_db_rows_use(db._h, ids[5]) == -1 and lib.vq_db_rows_drop(db._h, ids[5]) == -1           # gone
    rc, msg = define([1, 2])
    assert rc == 0 and vid.value == ids[5]                                       # its slot is used again
    # switching invalidates what the handle holds: the results cover another population
    db.set_query_from_row(3)
    db.scan(weights=[1.0])                                                       # (the handle was switched behind the Python object's back)
    buf = np.full(100, -7.0)
    assert lib.vq_db_read_scores(db._h, buf.ctypes.data_as(C.c_void_p)) == 0
    assert (buf[:6] != -7.0).all() and (buf[6:] == -7.0).all()                   # M = 6 scores came back, nothing behind them was touched
    assert lib.vq_db_rows_use(db._h, ids[4]) == 0 and lib.vq_db_read_scores(db._h, buf.ctypes.data_as(C.c_void_p)) == 0      # no change: results kept
    assert lib.vq_db_rows_use(db._h, -1) == 0
    assert lib.vq_db_read_scores(db._h, buf.ctypes.data_as(C.c_void_p)) == -4 and "no scores" in lib.vq_last_error().decode()
    db.close()


# ---------------------------------------------------------------------------------------------------------------- 6. tickets
def test_two_tickets_with_their_own_search_sets_share_one_database(vqa):
    from _search_set_cases import check_two_tickets
    g = golden_json("real_subset.json")
    x = golden_npy("real_subset_x.npy")
    ids = np.asarray(g.get("clip_ids") or g["clip_order"], dtype=np.int64)
    recs = records_from_dense(x, ids, [1, 2, 3])
    shared = vqa.FeatureDB.from_arrays(x, clip_ids=ids)
    calls = []
    real = vqa.feature_db.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)
    vqa.feature_db.call = counting
    try:
        check_two_tickets(vqa, shared, lambda rows: vqa.FeatureDB.from_arrays(x[rows], clip_ids=ids[rows]), recs, x, ids, g, STREAMS,
                          DEFAULT_WEIGHTS, SEED)
    finally:
        vqa.feature_db.call = real
    assert calls.count("vq_db_rows_define") == 2 and calls.count("vq_db_rows_drop") == 2
    assert 8 <= calls.count("vq_db_rows_use") <= 40                              # one per hand-back; none while the set does not change
    shared.close()
