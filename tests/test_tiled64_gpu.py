"""GPU: VQ_LAYOUT_TILED64, the tiled layout of float64 databases ([tile of 16 clips][S*E][D/2][clip][2]; vq_db_set_layout,
FeatureDB.set_layout("tiled64")), against a row-major float64 twin of the same seed, the oracle and the reference's goldens.

Tolerances are the project's (tests/test_sim_gpu.py): |delta| <= 1e-12 on dots and averaged similarities (the k order of a dot differs
between the layouts), scores bit-exact GIVEN the averages, ranks and partitions identical.  The 16-query pass runs the MFMA sequence of
the rows per (clip, query), so everything it returns is compared with ``==``.

Databases are generated on the device (FeatureDB.synthetic); rows are regenerated on the host only where sampled."""
import os

import numpy as np
import pytest

import sim_oracle as so
from _helpers import GOLDEN, golden_json, golden_npy, golden_target_array
from _scan_matrix_cases import D, MASKED, SCALES, SHAPES, TOL, WEIGHTS, check_sampled, one_hot_rows, sample_positions, shape_line, tile_view_rows
from _search_set_cases import np_select, presence_mask, same_bits, same_values

pytestmark = pytest.mark.gpu
F64 = np.float64


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


@pytest.fixture(scope="module")
def cus(gpu):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def waves(cus, s, e):
    """The rule of tests/_scan_matrix_cases.py::waves (launch_scan_t): workgroups of 4 waves, as many per compute unit as fit its
    160 KiB of LDS next to the fp64 query image (S E 8 KiB at D = 1024), 8 at the most."""
    per_cu = max(1, min(8, (160 * 1024) // (s * e * D * 8)))
    return cus * per_cu * 4


def _mask(n, s, e):
    """test_tiled_layout_in_place's: missing splits, every (clip, stream) keeping at least one"""
    present = np.ones((n, s, e), dtype=np.uint8)
    present[::5, 0, 0] = 0
    present[n - 1, :, e - 1] = 0
    present[..., 0] |= (present.sum(axis=2) == 0).astype(np.uint8)
    return present


# tests/test_sim_gpu.py::test_tiled_layout_in_place's list (16, 33: whole and ragged last tiles; 4 100 x (2, 4): past the 256 MB chunk of
# the conversion, 256 tiles of 1 MB; 70 003 and 140 007: more than 8 192 tiles, a second round per workgroup of the 16-query pass) plus
# one clip and one clip past a tile
@pytest.mark.parametrize("n,s,e,q,masked", [(70_003, 2, 3, 16, False), (5_001, 1, 2, 7, True), (33, 2, 5, 16, False), (140_007, 2, 1, 16, True),
                                            (16, 1, 1, 1, False), (4_100, 2, 4, 9, True), (1, 2, 2, 3, False), (17, 1, 3, 16, True)])
def test_tiled64_layout_in_place(vqa, n, s, e, q, masked):
    """set_layout("tiled64") turns the block of a float64 database into [tile][slice][k / 2][clip][2] IN PLACE.  On it the 16-query
    pass has the bits of the pass on the rows; the one-query scan agrees with the row-major scan and with the oracle to <= 1e-12 and
    is bit-reproducible; rows read back, the query made from a row, uploads into the middle and the ragged end and target
    bootstrapping see the same data; converting back restores the block bit for bit."""
    d = 1024
    rng = np.random.default_rng(n + e)
    targets = rng.standard_normal((q, s, e, d)) / d
    weights = 0.5 + rng.random((q, s))
    present = _mask(n, s, e) if masked else None
    scales = (4.0, 1.0)[:s]
    plain = vqa.FeatureDB.synthetic(n, s, e, d, seed=29, scales=scales, dtype=F64)
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=29, scales=scales, dtype=F64)
    for h in (plain, db):
        h.set_present(present)
    assert db.layout == "rows" and db.tiled_layout == "tiled64"
    db.set_layout("tiled64")
    assert db.layout == "tiled64" and plain.layout == "rows"
    pick = np.array(sorted({0, n - 1, n // 2, min(17, n - 1), (n // 16) * 16 - 1 if n >= 16 else 0}))
    assert same_bits(db.read_rows(pick), plain.read_rows(pick))

    def both(fn):
        return fn(plain), fn(db)
    want, got = both(lambda h: h.scan_batch(targets, weights))
    assert (got == want).all() and (db.scan_batch(targets, weights) == got).all()
    t_rows, t_tiled = both(lambda h: h.set_query_from_row(int(pick[-1])))
    assert (t_rows == t_tiled).all()
    w1 = [1.0, 1.5][:s]
    for h in (plain, db):
        h.scan(weights=w1, keep_sims=True)
    (avg_r, ne_r, sims_r), (avg_t, ne_t, sims_t) = both(lambda h: h.similarities(sims=True))
    d_avg, d_sims = np.abs(avg_r - avg_t).max(), np.abs(sims_r - sims_t).max()
    print("n = %d: |avg tiled64 - rows| %.3g, |sims| %.3g" % (n, d_avg, d_sims))
    assert (ne_r == ne_t).all() and d_avg <= 1e-12 and d_sims <= 1e-12
    if n <= 6000:
        x = so.synth_features(29, 0, n, s, e, d, scales).astype(F64)
        o_sims, o_avg, o_ne = so.dense_similarities(x, t_rows, present)
        assert (ne_t == o_ne).all() and np.abs(avg_t - o_avg).max() <= 1e-12 and np.abs(sims_t - o_sims).max() <= 1e-12
    sc_t = db.scores()
    assert (sc_t == so.dense_scores(avg_t, w1)).all()                   # scores bit-exact given the averages, as on the rows
    db.scan(weights=w1, keep_sims=True)
    assert (db.scores() == sc_t).all() and (db.similarities()[0] == avg_t).all()
    if n >= 40 and not masked:
        v, iv = [int(pick[1]), 3, 20], [5, 30]
        b_r, b_t = both(lambda h: h.bootstrap_target(v, iv, mu=0.3, set_query=False))
        assert (b_r == b_t).all()
    # new float64 rows in the middle and at the ragged end, through vq_db_upload: dealt into their tiles
    rows = rng.random((40, s, e, d)) * 3
    for h in (plain, db):
        h.upload(max(0, n // 2 - 10), rows[:min(25, n)])
        h.upload(max(0, n - 15), rows[25:25 + min(15, n)])
    want2, got2 = both(lambda h: h.scan_batch(targets, weights))
    assert not (want2 == want).all() and (got2 == want2).all()
    with pytest.raises(vqa.VqError):
        db.feats_devptr()                                              # a tiled block is not [N][S][E][D]
    db.set_layout("rows")
    assert db.layout == "rows"
    head, tail = np.arange(min(n, 64)), np.arange(max(0, n - 40), n)
    assert same_bits(db.read_rows(head), plain.read_rows(head)) and same_bits(db.read_rows(tail), plain.read_rows(tail))
    for h in (plain, db):
        h.set_query(t_rows)
        h.scan(weights=w1)
    assert (plain.scores() == db.scores()).all()                       # back on the rows: the row-major scan's own bits
    plain.close()
    db.close()


def _scan(db, w):
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    return avg, n_e, sims, db.scores()


@pytest.mark.parametrize("s,e", SHAPES)
def test_every_shape_of_the_tiled64_scan_with_more_tiles_than_waves(vqa, cus, s, e):
    """n = 16 (2 W) + 5 clips: 2 W + 1 tiles on W waves, the last tile holds 5 clips (2.1 - 5.4 GB of float64).  The tiled64 handle
    against a row-major one of the same seed (n_e equal, avg and sims <= 1e-12) and both against the oracle on sampled rows; scores bit
    for bit from the tiled avg; a second scan the same bits; a view with untouched tiles, tiles touched in one clip and the ragged last
    tile == the tiled64 full scan at its rows, bit for bit.  The MASKED shape of each S again under a presence mask that leaves
    (clip, stream) pairs without a split."""
    W = waves(cus, s, e)
    n = 16 * (2 * W) + 5
    ntiles = (n + 15) // 16
    assert ntiles > 2 * W and n % 16 == 5
    seed, w = 300 + 10 * s + e, WEIGHTS[:s]
    t = np.random.default_rng(seed).standard_normal((s, e, D)) / D
    rows_db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s], dtype=F64)
    rows_db.set_query(t)
    r_avg, r_ne, r_sims, r_sc = _scan(rows_db, w)
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s], dtype=F64)
    db.set_layout("tiled64")
    assert db.layout == "tiled64"
    db.set_query(t)
    full = _scan(db, w)
    avg, n_e, sims, sc = full
    assert (n_e == r_ne).all() and (n_e == e).all()
    assert np.abs(avg - r_avg).max() <= TOL and np.abs(sims - r_sims).max() <= TOL
    at = sample_positions(n)
    err_t = check_sampled(seed, s, e, F64, t, at, sims[at], avg[at], n_e[at])
    err_r = check_sampled(seed, s, e, F64, t, at, r_sims[at], r_avg[at], r_ne[at])
    assert (sc == so.dense_scores(avg, w)).all() and (r_sc == so.dense_scores(r_avg, w)).all()
    assert all(same_bits(a, b) for a, b in zip(_scan(db, w), full)), "second scan"
    rows = tile_view_rows(n, seed)
    touched = np.unique(rows >> 4).size
    assert W < touched < ntiles                                # view waves walk a second tile too
    db.define_search_rows("v", rows)
    db.use_search_set("v")
    got = _scan(db, w)
    assert got[0].shape == (rows.size, s) and got[2].shape == (rows.size, s, e)
    assert all(same_bits(a, b[rows]) for a, b in zip(got, full)), "view"
    db.use_search_set(None)
    masked = ""
    if MASKED[s] == (s, e):
        present = presence_mask(n, s, e)
        assert (present[1, 0] == 0).all() and (present[n - 1, s - 1] == 0).all()
        for h in (rows_db, db):
            h.set_present(present)
        m_full = _scan(db, w)
        m_avg, m_ne, m_sims, m_sc = m_full
        mr_avg, mr_ne, mr_sims, _ = _scan(rows_db, w)
        assert (m_ne == present.sum(axis=2)).all() and (m_ne == mr_ne).all() and (np.isnan(m_avg) == (m_ne == 0)).all()
        assert (np.isnan(mr_avg) == np.isnan(m_avg)).all()
        fin = ~np.isnan(m_avg)
        assert np.abs(m_avg[fin] - mr_avg[fin]).max() <= TOL and np.abs(m_sims - mr_sims).max() <= TOL
        check_sampled(seed, s, e, F64, t, at, m_sims[at], m_avg[at], m_ne[at], present)       # rows 1 and n - 1 are among them
        assert same_values(m_sc, so.dense_scores(m_avg, w)) and (np.isnan(m_sc) == (m_ne == 0).any(axis=1)).all()
        assert all(same_bits(a, b) for a, b in zip(_scan(db, w), m_full)), "second masked scan"
        db.use_search_set("v")
        m_got = _scan(db, w)
        assert all(same_bits(a, b[rows]) for a, b in zip(m_got, m_full)), "masked view"
        masked = ", masked"
    print("%s tiled64 n = %d, %d tiles on %d waves, view of %d rows in %d tiles, |d| tiled64 %.3g rows %.3g%s" % (
        shape_line(s, e), n, ntiles, W, rows.size, touched, err_t, err_r, masked))
    rows_db.close()
    db.close()


def test_one_hot_rows_are_exact_on_tiled64(vqa):
    """Rows whose dots are one exact product (one_hot_rows): the similarities equal the oracle's with ``==`` in every order of the sum,
    for every (S, E) of the dispatch."""
    for s, e in SHAPES:
        x, t = one_hot_rows(1024, s, e, F64)
        db = vqa.FeatureDB.from_arrays(x)
        db.set_layout("tiled64")
        db.set_query(t)
        db.scan(weights=WEIGHTS[:s], keep_sims=True)
        avg, n_e, sims = db.similarities(sims=True)
        o_sims, o_avg, o_ne = so.dense_similarities(x, t, None)
        assert (sims == o_sims).all() and (n_e == o_ne).all(), (s, e)
        db.close()


def _golden_case(name):
    g = golden_json(name + ".json")
    x = golden_npy(name + "_x.npy")
    ids = np.asarray(g.get("clip_ids") or g["clip_order"])
    present = np.array(g["present"], dtype=np.uint8) if "present" in g else None
    pos = {int(c): i for i, c in enumerate(ids)}
    rows = [pos[c] for c in g["clip_order"]]
    return g, x[rows], np.asarray(g["clip_order"]), (present[rows] if present is not None else None)


def _nan_array(v):
    return np.array([np.nan if a is None else a for a in np.asarray(v, dtype=object).reshape(-1)], dtype=F64).reshape(np.shape(v))


def _same_ranks(a, b):
    """all ranks: the stable descending order (NaN last) of a is that of b"""
    return (np.argsort(-a, kind="stable") == np.argsort(-b, kind="stable")).all()


@pytest.mark.parametrize("name", ["real_subset", "synth_small", "ragged"])
def test_reference_goldens_stored_as_float64_and_tiled(vqa, name):
    """avg and scores <= 1e-12 from the reference's recorded values; all ranks identical (the smallest gap between neighbouring golden
    scores -- 3.6e-4, 2.5e-6, 1.4e-4 -- is far above twice the tolerance)."""
    g, x, ids, present = _golden_case(name)
    db = vqa.FeatureDB.from_arrays(x.astype(F64), clip_ids=ids, present=present)
    db.set_layout("tiled64")
    assert db.layout == "tiled64"
    db.set_query(golden_target_array(g))
    db.scan(weights=[1.0, 1.5])
    avg, n_e = db.similarities()
    assert (n_e == np.array(g["sim_n"])).all()
    g_avg = _nan_array(g["sim_avg"])
    ok = ~np.isnan(g_avg)
    assert np.abs(avg[ok] - g_avg[ok]).max() <= 1e-12 and np.isnan(avg[~ok]).all()
    sc, g_sc = db.scores(), _nan_array(g["scores_default"])
    fin = ~np.isnan(g_sc)
    assert (np.isnan(sc) == ~fin).all() and np.abs(sc[fin] - g_sc[fin]).max() <= 1e-12
    assert same_values(sc, so.dense_scores(avg, [1.0, 1.5]))
    assert _same_ranks(sc, g_sc)
    db.close()


def test_cfg1_10k_stored_as_float64_and_tiled(vqa):
    """tests/test_sim_gpu.py::test_cfg1_10k_against_reference on a tiled64 database: the smallest gap between neighbouring golden
    scores is 7.8e-11, above twice the tolerance, so all 10 000 ranks, the select and the top-k are the reference's."""
    z = np.load(os.path.join(GOLDEN, "cfg1_10k.npz"))
    meta = golden_json("cfg1_10k.json")
    x = so.cfg1_features(n=10000, e=3, seed=0)
    db = vqa.FeatureDB.from_arrays(x.astype(F64))
    db.set_layout("tiled64")
    t = np.stack([[so.scale_feature(x[7, s, e].astype(np.float64)) for e in range(3)] for s in range(2)])
    db.set_query(t)
    db.scan(weights=[1.0, 1.5])
    avg, n_e = db.similarities()
    assert (n_e == 3).all()
    assert np.abs(avg - z["sim_avg"]).max() <= 1e-12
    sc = db.scores()
    assert np.abs(sc - z["scores_default"]).max() <= 1e-12
    assert _same_ranks(sc, z["scores_default"])                        # all 10k ranks
    m, r, amax = db.select(0.8, 0.8 - 0.35 * 0.2)
    assert [int(db.clip_ids[i]) for i in m] == [c for c, _ in meta["select_default"]]
    rows, vals = db.topk(100)
    o_rows, o_vals = so.dense_topk(z["scores_default"], 100)
    assert (rows == o_rows).all()
    db.rescore([1.0, meta["opt_weights"]["warped_optical_flow"]])
    assert np.abs(db.scores() - z["scores_opt"]).max() <= 1e-12
    db.close()


def _band(scores, lo_q, hi_q):
    """(threshold, lower) in the middle of the widest gaps between neighbouring scores around two quantiles: no score near an edge"""
    v = np.sort(scores[~np.isnan(scores)])

    def edge(qu):
        i = int(qu * (v.size - 1))
        a = v[max(0, i - 20):i + 21]
        k = int(np.argmax(np.diff(a)))
        return 0.5 * (a[k] + a[k + 1])
    return edge(hi_q), edge(lo_q)


def _same_result(a, b):
    return all(same_bits(getattr(a, f), getattr(b, f)) for f in ("avg", "n_e", "scores", "match_rows", "near_rows")) and a.near_argmax == b.near_argmax


@pytest.mark.parametrize("masked", [False, True])
def test_rounds_on_tiled64_against_the_row_major_twin(vqa, masked):
    """5 001 clips x 2 x 3: query_round (<= 1e-12, equal partitions: the bands are placed so that no score of either handle lies within
    2e-12 of an edge, which is asserted), query_round_batch and query_round_batch_sets (sets of tile_view_rows, an empty set and a
    whole-database member) with ``==`` on every array."""
    n, s, e, q = 5_001, 2, 3, 7
    rng = np.random.default_rng(77)
    present = _mask(n, s, e) if masked else None
    plain = vqa.FeatureDB.synthetic(n, s, e, D, seed=41, scales=SCALES, dtype=F64)
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=41, scales=SCALES, dtype=F64)
    for h in (plain, db):
        h.set_present(present)
    db.set_layout("tiled64")
    t = plain.set_query_from_row(11)
    w = np.array([1.0, 1.5])
    probe = plain.query_round(t, weights=w)
    th, lower = _band(np.array(probe.scores), 0.90, 0.97)
    r_r, r_t = plain.query_round(t, weights=w, select=(th, lower)), db.query_round(t, weights=w, select=(th, lower))
    for r in (r_r, r_t):
        assert np.abs(np.array(r.scores) - th).min() > 2e-12 and np.abs(np.array(r.scores) - lower).min() > 2e-12
    assert (np.array(r_r.n_e) == np.array(r_t.n_e)).all()
    assert np.abs(np.array(r_r.avg) - np.array(r_t.avg)).max() <= 1e-12 and np.abs(np.array(r_r.scores) - np.array(r_t.scores)).max() <= 1e-12
    assert (np.array(r_t.scores) == so.dense_scores(np.array(r_t.avg), w)).all()
    assert len(r_t.match_rows) > 0 and len(r_t.near_rows) > 0
    assert (np.array(r_r.match_rows) == np.array(r_t.match_rows)).all() and (np.array(r_r.near_rows) == np.array(r_t.near_rows)).all()
    assert r_r.near_argmax == r_t.near_argmax
    want = np_select(np.array(r_t.scores), th, lower)
    assert (np.array(r_t.match_rows) == want[0]).all() and (np.array(r_t.near_rows) == want[1]).all() and r_t.near_argmax == want[2]
    # batched rounds: the MFMA sequence of the rows, so the same bits everywhere
    targets = rng.standard_normal((q, s, e, D)) / D
    targets[0] = t
    weights = 0.5 + rng.random((q, s))
    ref = plain.query_round_batch(targets, weights, None)
    bands = np.array([np.quantile(ref[i].scores, [0.97, 0.90]) for i in range(q)])
    b_r, b_t = plain.query_round_batch(targets, weights, bands), db.query_round_batch(targets, weights, bands)
    assert len(b_t) == q and all(_same_result(a, b) for a, b in zip(b_r, b_t))
    assert all(len(r.match_rows) > 0 and len(r.near_rows) > 0 for r in b_t)
    sets = {"a": tile_view_rows(n, 3), "b": tile_view_rows(n, 4)[::2], "none": np.zeros(0, dtype=np.int64)}
    for h in (plain, db):
        for name, rows in sets.items():
            h.define_search_rows(name, rows)
    set_ids = ["a", "b", "none", None, "a", "b", "none"]
    v_r, v_t = (h.query_round_batch_sets(targets, weights, set_ids, bands) for h in (plain, db))
    assert all(_same_result(a, b) for a, b in zip(v_r, v_t))
    for i, sid in enumerate(set_ids):
        rows = np.arange(n) if sid is None else sets[sid]
        assert v_t[i].scores.shape == (rows.size,) and same_bits(v_t[i].scores, b_t[i].scores[rows]) and same_bits(v_t[i].avg, b_t[i].avg[rows])
    plain.close()
    db.close()


def test_tiled64_is_refused_where_it_cannot_hold(vqa):
    """Each storage type has one tiled layout: "tiled64" on float32 / float16 and "tiled" on float64 are VQ_E_UNSUPPORTED (-5), as are
    shapes without a tiled scan kernel; a block whose address was handed out is VQ_E_STATE (-4).  The handle works after each."""
    rng = np.random.default_rng(8)

    def works(db):
        tg = rng.standard_normal((2, db.S, db.E, db.D)) / db.D
        assert np.isfinite(db.scan_batch(tg, np.ones((2, db.S)))).all() and db.layout == "rows"
    for layout, kw in (("tiled64", {"dtype": np.float32}), ("tiled64", {"dtype": np.float16}), ("tiled", {"dtype": F64}),
                       ("tiled64", {"dim": 256}), ("tiled64", {"n_streams": 3})):
        args = dict(n=200, n_streams=2, n_splits=2, dim=1024, dtype=F64)
        args.update(kw)
        db = vqa.FeatureDB.synthetic(args["n"], args["n_streams"], args["n_splits"], args["dim"], seed=3, scales=(2.0, 1.0, 1.0)[:args["n_streams"]],
                                     dtype=args["dtype"])
        with pytest.raises(vqa.VqError) as ei:
            db.set_layout(layout)
        assert ei.value.code == -5, (layout, kw)
        assert db.tiled_layout == (None if (kw.get("dtype") == np.float16 or "dim" in kw or "n_streams" in kw) else
                                   "tiled" if kw.get("dtype") == np.float32 else "tiled64")
        works(db)
        db.close()
    db = vqa.FeatureDB.synthetic(200, 2, 2, 1024, seed=31, scales=(2.0, 1.0), dtype=F64)
    db.feats_devptr()                                                  # from here on others may write the rows
    with pytest.raises(vqa.VqError) as ei:
        db.set_layout("tiled64")
    assert ei.value.code == -4
    works(db)
    with pytest.raises(KeyError):
        db.set_layout("tiled128")                                      # a name that is no layout never reaches the library
    db.close()


def test_csv_tree_into_tiled64(vqa, tmp_path):
    """from_csv_tree(layout="tiled64", dtype=float64): the values land in their tiles; read_rows equals the "rows" load bit for bit."""
    from video_query_algorithms_amd.tsn import feature_csv
    rng = np.random.default_rng(64)
    nclips = 37                                                        # two whole tiles and a ragged one
    feats = {m: (rng.random((nclips, 25, 1024)).astype(np.float32) * np.float32(2.0)).astype(F64).mean(axis=1) for m in feature_csv.STREAM_MODES}
    names = ["clip_%04d" % (i + 1) for i in range(nclips)]
    for split in (1, 2):
        feature_csv.write_features(str(tmp_path / "features"), "video_a", "/a/video_a.mp4", "UCF101_split%d" % split, "global_pool", names,
                                   feats, {m: m + ".caffemodel" for m in feature_csv.STREAM_MODES})
    rows_db = vqa.FeatureDB.from_csv_tree(str(tmp_path / "features"), dtype=F64)
    tiled = vqa.FeatureDB.from_csv_tree(str(tmp_path / "features"), dtype=F64, layout="tiled64")
    assert tiled.layout == "tiled64" and rows_db.layout == "rows" and (tiled.n, tiled.S, tiled.E, tiled.D) == (nclips, 2, 2, 1024)
    got, want = tiled.read_rows(np.arange(nclips)), rows_db.read_rows(np.arange(nclips))
    assert same_bits(got, want)
    for si, m in enumerate(feature_csv.STREAM_MODES):
        for ei in range(2):
            assert same_bits(got[:, si, ei], feats[m])
    rows_db.close()
    tiled.close()
