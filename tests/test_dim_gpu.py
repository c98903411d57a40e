"""GPU: feature databases of any vector length d on rows stored at a zero-padded pitch D (include/vq_amd_dim.h: flag bits of vq_db_create; FeatureDB.D / .Dp),
and the short-row scan kernel (scan_short_kernel, csrc/vq_sim.hip).

Tolerances (stated once):
  * a database padded by the library against the same data padded by hand, both on scan_generic_kernel: EQUAL (the same kernel on
    the same bytes; tests/_dim_child.py, a process of its own because VQ_SCAN_SHORT is read once);
  * the short-row kernel against the oracle: |delta| <= SIM_TOL = 1e-12, the bound every scan of tests/test_sim_gpu.py is held to --
    at most 128 fp64 terms of magnitude <= 1 summed in another order than numpy's differ by about 1e-14; n_e is compared with ==;
    scores GIVEN the device's averages are bit-exact against oracle.dense_scores;
  * stored D = 1024 (d = 1023): rows against the oracle and tiled against rows 1e-12, as tests/test_sim_gpu.py's tiled test;
  * rows read back, file routes, re-uploads: EQUAL."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sim_oracle as so
from _dim_cases import draw, padded, same, target_of
from _helpers import STREAMS, records_from_dense

pytestmark = pytest.mark.gpu
SIM_TOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [np.float32, np.float64, np.float16]


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


# ---------------------------------------------------------------------------------------------- 1. padded by the library == by hand
@pytest.mark.parametrize("dtype", ["float32", "float64", "float16"])
def test_padded_by_the_library_equals_padded_by_hand(gpu, dtype):
    env = dict(os.environ, VQ_SCAN_SHORT="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_dim_child.py"), dtype], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "42 cases" in r.stdout, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------- 2. the short-row kernel
def _short_db(vqa, x, present=None, dtype=None):
    """The database of x on a handle with the short-rows flag (this process does not set VQ_SCAN_SHORT: the short-row kernel runs)."""
    assert os.environ.get("VQ_SCAN_SHORT") in (None, "1")
    n, s, e, d = x.shape
    db = vqa.FeatureDB(n, s, e, d, x.dtype if dtype is None else dtype, short_rows=True)
    db.upload(0, x)
    if present is not None:
        db.set_present(present)
    return db


def _check_against_oracle(db, x, t, present, rows=None, w=(1.0, 1.5)):
    w = list(w)[:db.S]
    db.set_query(t)
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    sel = slice(None) if rows is None else rows
    o_sims, o_avg, o_ne = so.dense_similarities(x.astype(np.float64)[sel], t, None if present is None else present[sel])
    assert (n_e == o_ne).all()
    err_s = np.abs(sims - o_sims).max()
    ok = o_ne > 0
    err_a = np.abs(avg[ok] - o_avg[ok]).max() if ok.any() else 0.0
    print("short rows %s n=%d S=%d E=%d d=%d: sims |d| = %.3g, avg |d| = %.3g" % (x.dtype.name, x.shape[0], db.S, db.E, db.D, err_s, err_a))
    assert err_s <= SIM_TOL and err_a <= SIM_TOL
    assert np.isnan(avg[~ok]).all()
    sc = db.scores()
    assert np.array_equal(sc, so.dense_scores(avg, w), equal_nan=True)         # bit-exact given the same avg
    return avg, n_e, sims, sc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [3, 8, 9, 101, 125])                             # stored D = 4, 8, 12, 104, 128: L = 1, 2, 4, 32, 32
def test_short_kernel_against_the_oracle(vqa, d, dtype):
    rng = np.random.default_rng(d)
    for n in (1, 63, 64, 65):
        x, present, rows, t = draw(rng, n, 2, 3, d, dtype)
        if n == 65:
            present[7, 1, :] = 0                                               # one stream of one clip is empty: n_e = 0, avg NaN
        db = _short_db(vqa, x, present)
        assert (db.D, db.Dp) == (d, (d + 3) // 4 * 4) and db.Dp <= 128
        full = _check_against_oracle(db, x, t, present)
        if n == 65:
            assert full[1][7, 1] == 0 and np.isnan(full[0][7, 1]) and np.isnan(full[3][7])
        # under a row view: results at positions, presence bits by database row -- the full scan's bits
        db.define_search_rows("set", rows)
        db.use_search_set("set")
        part = _check_against_oracle(db, x, t, present, rows)
        for a, b in zip(part, full):
            assert same(a, b[rows])
        db.close()


@pytest.mark.parametrize("d,lanes", [(4, 1), (101, 32)])
def test_short_kernel_walks_the_grid_twice_with_a_ragged_tail(vqa, d, lanes):
    """One N just past a full grid per extreme of L: 256 CUs x 8 workgroups x 4 waves x (64 / L) clips + 3."""
    n = 256 * 8 * 4 * (64 // lanes) + 3
    s, e = (1, 1) if lanes == 1 else (2, 3)
    rng = np.random.default_rng(n)
    x = np.abs(rng.standard_normal((n, s, e, d), dtype=np.float32))
    assert x.nbytes <= 50 << 20
    t = target_of(x, n - 2)
    db = _short_db(vqa, x)
    avg, _n_e, _sims, sc = _check_against_oracle(db, x, t, None)
    assert np.abs(avg[n - 2] - 1.0).max() <= 1e-14 and abs(sc[n - 2] - 1.0) <= 1e-14
    rows = np.unique(np.concatenate([rng.integers(0, n, 5000), np.arange(n - 5, n)])).astype(np.int64)
    db.define_search_rows("set", rows)
    db.use_search_set("set")
    part = _check_against_oracle(db, x, t, None, rows)
    assert same(part[0], avg[rows]) and same(part[3], sc[rows])
    db.close()


def test_short_kernel_with_a_query_of_64_kb(vqa):
    """(S, E) = (8, 8), d = 125: the LDS image of the query is 64 x 128 doubles."""
    rng = np.random.default_rng(125)
    x, present, rows, t = draw(rng, 65, 8, 8, 125, np.float64)
    db = _short_db(vqa, x, present)
    _check_against_oracle(db, x, t, present, w=np.linspace(0.5, 2.0, 8))
    db.define_search_rows("set", rows)
    db.use_search_set("set")
    _check_against_oracle(db, x, t, present, rows, w=np.linspace(0.5, 2.0, 8))
    db.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_short_kernel_on_101_equals_short_kernel_on_a_hand_padded_104(vqa, dtype):
    rng = np.random.default_rng(104)
    x, present, rows, t = draw(rng, 130, 2, 3, 101, dtype)
    lib, hand = _short_db(vqa, x, present), _short_db(vqa, padded(x, 104), present)
    assert (lib.D, lib.Dp, hand.D, hand.Dp) == (101, 104, 104, 104)
    lib.set_query(t)
    hand.set_query(padded(t, 104))
    for db in (lib, hand):
        db.scan(weights=[1.0, 1.5], keep_sims=True)
    for a, b in zip(lib.similarities(sims=True) + (lib.scores(),), hand.similarities(sims=True) + (hand.scores(),)):
        assert same(a, b)
    # and the generic kernel on the same rows (a padded handle without the short-rows flag) agrees to rounding, with the same n_e
    short = lib.similarities()
    plain = vqa.FeatureDB(130, 2, 3, 101, dtype, short_rows=False)
    plain.upload(0, x)
    plain.set_present(present)
    plain.set_query(t)
    plain.scan(weights=[1.0, 1.5])
    generic = plain.similarities()
    assert (short[1] == generic[1]).all() and np.abs(short[0] - generic[0]).max() <= SIM_TOL
    for db in (lib, hand, plain):
        db.close()


def test_padding_is_asked_for_and_the_plain_constructor_is_what_it_was(vqa):
    """Without ``short_rows`` the constructor is vq_db_create as ever: a length that is no multiple of 4 is refused.  With it the handle
    stores at the pitch, which vq_db_shape answers."""
    for dim in (101, 1022):
        with pytest.raises(vqa.VqError) as ei:
            vqa.FeatureDB(8, 2, 3, dim)
        assert ei.value.code == -1 and "multiple of 4" in str(ei.value)
    D = C.c_int32()
    for dim, short_rows, pitch in ((104, None, 104), (104, True, 104), (101, True, 104), (101, False, 104), (129, True, 132), (1022, True, 1024)):
        db = vqa.FeatureDB(8, 2, 3, dim, short_rows=short_rows)
        vqa._lib.call("vq_db_shape", db._h, None, None, None, C.byref(D), None)
        assert (db.D, db.Dp, D.value) == (dim, pitch, pitch)
        db.close()
    wide = vqa.FeatureDB(8, 2, 3, 129, short_rows=True)                        # flagged, but D = 132 > 128: the generic kernel
    x = np.abs(np.random.default_rng(129).standard_normal((8, 2, 3, 129))).astype(np.float32)
    wide.upload(0, x)
    _check_against_oracle(wide, x, target_of(x, 2), None)
    with pytest.raises(ValueError):
        wide.scan_batch(np.zeros((1, 2, 3, 129)), np.ones((1, 2)))
    assert not wide.batch_round_supported()
    wide.close()


# ---------------------------------------------------------------------------------------------- 3. stored D = 1024
def test_1023_runs_the_fast_kernels_and_may_be_tiled(vqa):
    rng = np.random.default_rng(1023)
    x, present, rows, t = draw(rng, 33, 2, 3, 1023, np.float32)
    db = vqa.FeatureDB.from_arrays(x, present=present)
    assert (db.D, db.Dp) == (1023, 1024) and db.layouts == ("rows", "tiled") and db.tiled_layout == "tiled"
    before = db.read_rows(np.arange(33))
    assert same(before, x)
    on_rows = _check_against_oracle(db, x, t, present)
    db.set_layout("tiled")
    assert db.layout == "tiled"
    assert same(db.read_rows(np.arange(33)), before)
    db.set_query(t)
    db.scan(weights=[1.0, 1.5], keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    assert (n_e == on_rows[1]).all() and np.abs(sims - on_rows[2]).max() <= SIM_TOL and np.abs(avg - on_rows[0]).max() <= SIM_TOL
    db.upload(5, x[20:24])                                                     # unpadded rows into the tiles
    assert same(db.read_rows([5, 6, 7, 8, 4, 9]), x[[20, 21, 22, 23, 4, 9]])
    db.set_layout("rows")
    assert same(db.read_rows(np.arange(33))[[0, 5, 32]], x[[0, 20, 32]])
    db.close()


# ---------------------------------------------------------------------------------------------- 4. file routes
HEADER = "video =%s, video url =/a/%s.mp4, CNN stream =%s, feature blob =fc-action, caffe model =m.caffemodel\n"


@pytest.fixture(scope="module")
def action_tree(tmp_path_factory):
    """2 videos x 2 streams x 2 splits of 101 class scores, about 20 clips, one file missing, both number formats."""
    from video_query_algorithms_amd.tsn import feature_csv
    root = str(tmp_path_factory.mktemp("fc_action"))
    rng = np.random.default_rng(101)
    k = 0
    for video, clips in (("va", 11), ("vb", 9)):
        for split in (1, 2):
            for stream in feature_csv.STREAM_MODES:
                k += 1
                if (video, split, stream) == ("vb", 2, "rgb"):
                    continue                                                   # the missing file: its slots are absent and read as zeros
                x = rng.standard_normal((clips, 101)) * 10.0 ** rng.integers(-6, 4, (clips, 101))
                d = os.path.join(root, video, "model_split%d" % split)
                os.makedirs(d, exist_ok=True)
                with open(os.path.join(d, "%s_fc-action_features.csv" % stream), "wb") as f:
                    f.write((HEADER % (video, video, stream)).encode() + feature_csv.format_rows(x, np.arange(1, clips + 1), "repr" if k % 2 else "g12"))
    return root


@pytest.mark.parametrize("dtype", DTYPES)
def test_csv_tree_of_101_scores_equals_the_store_route(vqa, action_tree, tmp_path, dtype):
    from video_query_algorithms_amd.feature_store import open_store, store_from_csv_tree
    store = store_from_csv_tree(action_tree, str(tmp_path / "store"), dtype=dtype)
    _meta, feats, ids, present = open_store(store)
    assert feats.shape == (20, 2, 2, 101) and present is not None and not np.asarray(present).all()
    via_store = vqa.FeatureDB.from_store(store)
    db = vqa.FeatureDB.from_csv_tree(action_tree, dtype=dtype)
    for h in (db, via_store):
        assert h.dtype == np.dtype(dtype) and (h.n, h.S, h.E, h.D, h.Dp) == (20, 2, 2, 101, 104)
    got = db.read_rows(np.arange(20))
    assert got.tobytes() == np.ascontiguousarray(feats).tobytes() == via_store.read_rows(np.arange(20)).tobytes()
    assert (db.clip_ids == ids).all() and (db.present == np.asarray(present)).all() and db.csv_host_fields == 0
    assert db.stream_names == via_store.stream_names and db.slot_splits == via_store.slot_splits
    # the pads, through the raw call at pitch: +0.0 in every vector of both databases
    for h in (db, via_store):
        raw = np.empty((20, 2, 2, 104), dtype=dtype)
        r = np.arange(20, dtype=np.int64)
        vqa._lib.call("vq_db_read_rows", h._h, r.ctypes.data_as(C.c_void_p), 20, raw.ctypes.data_as(C.c_void_p))
        assert raw[..., :101].tobytes() == got.tobytes()
        assert not raw[..., 101:].view({2: np.uint16, 4: np.uint32, 8: np.uint64}[raw.itemsize]).any()
    # a file whose rows have another length than the database's logical one is refused, naming both
    with pytest.raises(vqa.VqError, match="104 values, the database's 101"):
        db.load_csv(b"h\n1," + b",".join([b"1.0"] * 104) + b"\n", 0, 0, [0])
    db.close()
    via_store.close()


# ---------------------------------------------------------------------------------------------- 5. the seam
def test_one_round_through_install_on_records_of_length_101(vqa):
    n, d, splits = 40, 101, [1, 2, 3]
    rng = np.random.default_rng(5)
    x = np.abs(rng.standard_normal((n, 2, 3, d)))
    ids = np.arange(100, 100 + n)
    recs = records_from_dense(x, ids, splits)

    class Hp:
        streams, feature_name = STREAMS, "global_pool"
        weights = {STREAMS[0]: 1.0, STREAMS[1]: 1.5}
        threshold, near_miss_default = 0.7, 0.2

    class Target:
        target_features = {st: {sp: so.scale_feature(x[3, si, ei]).tolist() for ei, sp in enumerate(splits)} for si, st in enumerate(STREAMS)}

    class Ticket:                                                              # the reference's class, as far as the seam touches it
        search_set = 1
        target = Target()

        def _request(self, action, params):
            assert action == ["search-sets", "features"]
            return recs

    vqa.install(Ticket)
    tk = Ticket()
    tk.compute_similarities(Hp())
    ahead = tk._ahead                                                          # the round came back in one call, lists included
    db = tk.feature_db
    assert (db.D, db.Dp, db.n, db.dtype) == (101, 104, n, np.dtype(np.float64))
    cand = {st: {sp: {int(c): x[i, si, ei].tolist() for i, c in enumerate(ids)} for ei, sp in enumerate(splits)} for si, st in enumerate(STREAMS)}
    want = so.faithful_similarities(Target.target_features, cand)
    assert list(tk.similarities.keys()) == list(want.keys())
    for c, entry in want.items():
        for st in STREAMS:
            assert abs(tk.similarities[c][st][0] - entry[st][0]) <= SIM_TOL and tk.similarities[c][st][1] == entry[st][1] == 3
    tk.compute_scores(Hp.weights)
    o_scores = so.faithful_scores(want, Hp.weights)
    assert list(tk.scores.keys()) == list(o_scores.keys())
    assert max(abs(tk.scores[c] - v) for c, v in o_scores.items()) <= SIM_TOL
    # the review partition is the oracle's on the device's scores
    near = Hp.near_miss_default
    lower = Hp.threshold - near * (1 - Hp.threshold)
    dev = db.scores()
    m_rows, n_rows, amax = db.select(Hp.threshold, lower)
    om, on, oa = so.dense_select_partition(dev, Hp.threshold, near)
    assert same(m_rows, om) and same(n_rows, on) and amax == oa and om.size >= 1
    assert ahead is not None and same(np.asarray(ahead["match_rows"]), om) and same(np.asarray(ahead["near_rows"]), on) and ahead["near_argmax"] == oa
    db.close()


# ---------------------------------------------------------------------------------------------- 6. re-upload
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_uploaded_over_other_rows_equal_a_fresh_handle(vqa, dtype):
    rng = np.random.default_rng(6)
    n, s, e, d = 50, 2, 3, 101
    first = np.abs(rng.standard_normal((n, s, e, d))).astype(np.float32).astype(dtype)
    x = np.abs(rng.standard_normal((n, s, e, d))).astype(np.float32).astype(dtype)
    fresh = vqa.FeatureDB.from_arrays(x, dtype=dtype)
    r = np.arange(n, dtype=np.int64)

    def raw_rows(db):
        out = np.empty((n, s, e, 104), dtype=dtype)
        vqa._lib.call("vq_db_read_rows", db._h, r.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p))
        return out
    want = raw_rows(fresh)
    assert same(want, padded(x, 104))
    # route 1: unpadded rows, padded on the device, in two pieces over the old data
    a = vqa.FeatureDB.from_arrays(first, dtype=dtype)
    a.upload(0, x[:17])
    a.upload(17, x[17:])
    assert raw_rows(a).tobytes() == want.tobytes()
    # route 2: a plain database of D = 104 (vq_db_create without flags), rows padded by the caller, over the old data
    b = vqa.FeatureDB.from_arrays(padded(first, 104), dtype=dtype)
    b.upload(0, padded(x, 104))
    assert raw_rows(b).tobytes() == want.tobytes()
    t = target_of(x, 3)
    res = []
    for db in (fresh, a, b):
        db.set_query(t if db.D == d else padded(t, 104))
        db.scan(weights=[1.0, 1.5])
        res.append((db.similarities()[0], db.scores()))
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])                              # the short-row kernel on the same bytes
    assert np.abs(res[0][0] - res[2][0]).max() <= SIM_TOL and np.abs(res[0][1] - res[2][1]).max() <= SIM_TOL      # the generic kernel
    for db in (fresh, a, b):
        db.close()
