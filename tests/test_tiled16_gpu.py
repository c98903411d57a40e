"""GPU: VQ_LAYOUT_TILED16, the tiled layout of float16 databases ([tile of 16 clips][S*E][D/8][clip][8]; vq_db_set_layout,
FeatureDB.set_layout("tiled16")), against a row-major float16 twin of the same seed and the oracle fed the same halves.

Tolerances are the project's (tests/test_sim_gpu.py): |delta| <= 1e-12 on dots and averaged similarities (the k order of a dot differs
between the layouts), scores bit-exact GIVEN the averages.  The 16-query pass runs the MFMA sequence of the fp16 rows per (clip, query),
so everything it returns -- and everything the batched-round calls make of it -- is compared with ``==``.

Databases are generated on the device (FeatureDB.synthetic, rounded to nearest even); rows are regenerated on the host only where
sampled.  The reference's goldens are compared between the two float16 handles, not with their recorded fp64 results (rounding the
features to binary16 moves those): tests/_tiled16_cases.py says how ranks are compared."""
import numpy as np
import pytest

import sim_oracle as so
from _scan_matrix_cases import D, MASKED, SCALES, SHAPES, TOL, WEIGHTS, check_sampled, one_hot_rows, sample_positions, shape_line, tile_view_rows, waves
from _search_set_cases import np_select, presence_mask, same_bits, same_values
from _tiled16_cases import CFG1_BAND, GAP, GOLDENS, MIN_KEPT, cfg1_case16, golden_case16, rank_order, rank_prefix

pytestmark = pytest.mark.gpu
F16 = np.float16


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


@pytest.fixture(scope="module")
def cus(gpu):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _mask(n, s, e):
    """tests/test_tiled64_gpu.py's: missing splits, every (clip, stream) keeping at least one"""
    present = np.ones((n, s, e), dtype=np.uint8)
    present[::5, 0, 0] = 0
    present[n - 1, :, e - 1] = 0
    present[..., 0] |= (present.sum(axis=2) == 0).astype(np.uint8)
    return present


# one clip, a whole tile, one clip past a tile, two tiles and a clip; 13 200 x (2, 5): 825 tiles of 320 KB, past the 819-tile run that fits
# the 256 MB conversion block; 70 003 and 140 007: more than 8 192 tiles, a second round per workgroup of the 16-query pass
@pytest.mark.parametrize("n,s,e,q,masked", [(1, 2, 2, 3, False), (16, 1, 1, 1, False), (17, 1, 3, 16, True), (33, 2, 5, 16, False),
                                            (5_001, 1, 2, 7, True), (13_200, 2, 5, 9, True), (70_003, 2, 3, 16, False), (140_007, 2, 1, 16, True)])
def test_tiled16_layout_in_place(vqa, n, s, e, q, masked):
    """set_layout("tiled16") turns the block of a float16 database into [tile][slice][k / 8][clip][8] IN PLACE.  On it the 16-query
    pass has the bits of the pass on the rows; the one-query scan agrees with the row-major scan and with the oracle to <= 1e-12 and
    is bit-reproducible; rows read back, the query made from a row, uploads into the middle and the ragged end and target
    bootstrapping see the same data; converting back restores the block bit for bit."""
    d = 1024
    rng = np.random.default_rng(n + e)
    targets = rng.standard_normal((q, s, e, d)) / d
    weights = 0.5 + rng.random((q, s))
    present = _mask(n, s, e) if masked else None
    scales = (4.0, 1.0)[:s]
    plain = vqa.FeatureDB.synthetic(n, s, e, d, seed=29, scales=scales, dtype=F16)
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=29, scales=scales, dtype=F16)
    for h in (plain, db):
        h.set_present(present)
    assert db.layout == "rows" and db.layouts == ("rows", "tiled16")
    if (n, s, e) == (13_200, 2, 5):
        assert (n + 15) // 16 > (256 << 20) // (16 * s * e * d * 2)      # more tiles than one run of the conversion block holds
    db.set_layout("tiled16")
    assert db.layout == "tiled16" and plain.layout == "rows"
    pick = np.array(sorted({0, n - 1, n // 2, min(17, n - 1), (n // 16) * 16 - 1 if n >= 16 else 0}))
    before = plain.read_rows(pick)
    assert before.dtype == F16 and same_bits(db.read_rows(pick), before)

    def both(fn):
        return fn(plain), fn(db)
    want, got = both(lambda h: h.scan_batch(targets, weights))
    assert (got == want).all() and (db.scan_batch(targets, weights) == got).all()
    t_rows, t_tiled = both(lambda h: h.set_query_from_row(int(pick[-1])))
    assert same_bits(t_rows, t_tiled)
    w1 = [1.0, 1.5][:s]
    for h in (plain, db):
        h.scan(weights=w1, keep_sims=True)
    (avg_r, ne_r, sims_r), (avg_t, ne_t, sims_t) = both(lambda h: h.similarities(sims=True))
    d_avg, d_sims = np.abs(avg_r - avg_t).max(), np.abs(sims_r - sims_t).max()
    print("n = %d: |avg tiled16 - rows| %.3g, |sims| %.3g" % (n, d_avg, d_sims))
    assert (ne_r == ne_t).all() and d_avg <= 1e-12 and d_sims <= 1e-12
    if n <= 6000:
        x = so.synth_features(29, 0, n, s, e, d, scales).astype(F16)
        assert same_bits(before, x[pick])                              # the device rounds like numpy: to nearest even
        o_sims, o_avg, o_ne = so.dense_similarities(x, t_rows, present)
        assert (ne_t == o_ne).all() and np.abs(avg_t - o_avg).max() <= 1e-12 and np.abs(sims_t - o_sims).max() <= 1e-12
    sc_t = db.scores()
    assert (sc_t == so.dense_scores(avg_t, w1)).all()                   # scores bit-exact given the averages, as on the rows
    db.scan(weights=w1, keep_sims=True)
    assert (db.scores() == sc_t).all() and (db.similarities()[0] == avg_t).all()
    if n >= 40 and not masked:
        v, iv = [int(pick[1]), 3, 20], [5, 30]
        b_r, b_t = both(lambda h: h.bootstrap_target(v, iv, mu=0.3, set_query=False))
        assert same_bits(b_r, b_t)
    # new rows in the middle and at the ragged end, through vq_db_upload (rounded to binary16 on the way in): dealt into their tiles
    rows = rng.random((40, s, e, d)) * 3
    for h in (plain, db):
        h.upload(max(0, n // 2 - 10), rows[:min(25, n)])
        h.upload(max(0, n - 15), rows[25:25 + min(15, n)])
    assert same_bits(db.read_rows(pick), plain.read_rows(pick)) and same_bits(plain.read_rows([n - 1])[0], rows[25 + min(15, n) - 1].astype(F16))
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
def test_every_shape_of_the_tiled16_scan_with_more_tiles_than_waves(vqa, cus, s, e):
    """n = 16 (2 W) + 5 clips: 2 W + 1 tiles on W waves (W by the rule of launch_scan_t), the last tile holds 5 clips (0.5 - 1.4 GB of
    float16).  The tiled16 handle against a row-major one of the same seed (n_e equal, avg and sims <= 1e-12) and both against the
    oracle on sampled rows; scores bit for bit from the tiled avg; a second scan the same bits; a view with untouched tiles, tiles
    touched in one clip and the ragged last tile == the tiled16 full scan at its rows, bit for bit.  The MASKED shape of each S again
    under a presence mask that leaves (clip, stream) pairs without a split."""
    W = waves(cus, s, e)
    n = 16 * (2 * W) + 5
    ntiles = (n + 15) // 16
    assert ntiles > 2 * W and n % 16 == 5
    seed, w = 300 + 10 * s + e, WEIGHTS[:s]
    t = np.random.default_rng(seed).standard_normal((s, e, D)) / D
    rows_db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s], dtype=F16)
    rows_db.set_query(t)
    r_avg, r_ne, r_sims, r_sc = _scan(rows_db, w)
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=seed, scales=SCALES[:s], dtype=F16)
    db.set_layout("tiled16")
    assert db.layout == "tiled16"
    db.set_query(t)
    full = _scan(db, w)
    avg, n_e, sims, sc = full
    assert (n_e == r_ne).all() and (n_e == e).all()
    assert np.abs(avg - r_avg).max() <= TOL and np.abs(sims - r_sims).max() <= TOL
    at = sample_positions(n)
    err_t = check_sampled(seed, s, e, F16, t, at, sims[at], avg[at], n_e[at])
    err_r = check_sampled(seed, s, e, F16, t, at, r_sims[at], r_avg[at], r_ne[at])
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
        check_sampled(seed, s, e, F16, t, at, m_sims[at], m_avg[at], m_ne[at], present)       # rows 1 and n - 1 are among them
        assert same_values(m_sc, so.dense_scores(m_avg, w)) and (np.isnan(m_sc) == (m_ne == 0).any(axis=1)).all()
        assert all(same_bits(a, b) for a, b in zip(_scan(db, w), m_full)), "second masked scan"
        db.use_search_set("v")
        m_got = _scan(db, w)
        assert all(same_bits(a, b[rows]) for a, b in zip(m_got, m_full)), "masked view"
        masked = ", masked"
    print("%s tiled16 n = %d, %d tiles on %d waves, view of %d rows in %d tiles, |d| tiled16 %.3g rows %.3g%s" % (
        shape_line(s, e), n, ntiles, W, rows.size, touched, err_t, err_r, masked))
    rows_db.close()
    db.close()


def test_one_hot_rows_are_exact_on_tiled16(vqa):
    """Rows whose dots are one exact product (one_hot_rows: 1 .. 2.5 in steps of 0.25, exact in binary16): the similarities equal the
    oracle's with ``==`` in every order of the sum, for every (S, E) of the dispatch."""
    for s, e in SHAPES:
        x, t = one_hot_rows(1024, s, e, F16)
        assert x.dtype == F16 and (x.astype(np.float64) == one_hot_rows(1024, s, e, np.float64)[0]).all()
        db = vqa.FeatureDB.from_arrays(x, dtype=F16)
        db.set_layout("tiled16")
        assert db.dtype == F16 and db.layout == "tiled16"
        db.set_query(t)
        db.scan(weights=WEIGHTS[:s], keep_sims=True)
        avg, n_e, sims = db.similarities(sims=True)
        o_sims, o_avg, o_ne = so.dense_similarities(x, t, None)
        assert (sims == o_sims).all() and (n_e == o_ne).all(), (s, e)
        db.close()


def _pair16(vqa, x16, ids=None, present=None):
    rows_db = vqa.FeatureDB.from_arrays(x16, clip_ids=ids, present=present, dtype=F16)
    db = vqa.FeatureDB.from_arrays(x16, clip_ids=ids, present=present, dtype=F16)
    db.set_layout("tiled16")
    assert db.layout == "tiled16" and rows_db.layout == "rows" and db.dtype == F16 == rows_db.dtype
    return rows_db, db


def _compare_ranked(rows_db, db, w):
    """avg, scores <= 1e-12 between the handles (NaN in the same places); the ranks equal on the settled prefix of the row-major scores,
    which keeps at least MIN_KEPT of them.  Returns (row-major scores, tiled scores, prefix)."""
    for h in (rows_db, db):
        h.scan(weights=w)
    (avg_r, ne_r), (avg_t, ne_t) = rows_db.similarities(), db.similarities()
    assert (ne_r == ne_t).all() and (np.isnan(avg_r) == np.isnan(avg_t)).all()
    ok = ~np.isnan(avg_r)
    assert np.abs(avg_t[ok] - avg_r[ok]).max() <= 1e-12
    sc_r, sc_t = rows_db.scores(), db.scores()
    fin = ~np.isnan(sc_r)
    assert (np.isnan(sc_t) == ~fin).all() and np.abs(sc_t[fin] - sc_r[fin]).max() <= 1e-12
    assert same_values(sc_t, so.dense_scores(avg_t, w))
    k = rank_prefix(sc_r)
    assert k >= MIN_KEPT * sc_r.size, (k, sc_r.size)                   # the premise: neighbours in rank more than 2e-12 apart
    assert (rank_order(sc_t)[:k] == rank_order(sc_r)[:k]).all()
    return sc_r, sc_t, k


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_goldens_stored_as_float16_and_tiled(vqa, name):
    """The golden's features rounded to binary16, on float16 rows and tiled: avg and scores <= 1e-12 between the two, the ranks
    identical wherever neighbouring row-major scores are more than 2e-12 apart."""
    x16, ids, present, t = golden_case16(name)
    rows_db, db = _pair16(vqa, x16, ids, present)
    for h in (rows_db, db):
        h.set_query(t)
    sc_r, _sc_t, k = _compare_ranked(rows_db, db, [1.0, 1.5])
    print("%s as float16: %d of %d ranks settled" % (name, k, sc_r.size))
    rows_db.close()
    db.close()


def test_cfg1_10k_stored_as_float16_and_tiled(vqa):
    """cfg1_10k rounded to binary16, the query made from the rounded row 7: avg, scores (default and re-weighted) <= 1e-12 against the
    float16 rows; the ranks, the select and the top-100 identical where the premise (asserted) holds."""
    x16, t = cfg1_case16()
    rows_db, db = _pair16(vqa, x16)
    for h in (rows_db, db):
        h.set_query(t)
    sc_r, sc_t, k = _compare_ranked(rows_db, db, [1.0, 1.5])
    th, lower = CFG1_BAND
    for sc in (sc_r, sc_t):
        assert np.abs(sc - th).min() > GAP and np.abs(sc - lower).min() > GAP         # no score of either handle near an edge
    (m_r, n_r, a_r), (m_t, n_t, a_t) = rows_db.select(th, lower), db.select(th, lower)
    assert len(m_r) > 0 and (np.array(m_r) == np.array(m_t)).all() and (np.array(n_r) == np.array(n_t)).all()
    near = np.sort(sc_r[np.array(n_r)])[::-1] if len(n_r) else np.zeros(0)
    if near.size > 1 and near[0] - near[1] > GAP:
        assert a_r == a_t
    top = min(100, k)
    (rows_r, vals_r), (rows_t, vals_t) = rows_db.topk(100), db.topk(100)
    assert (rows_r[:top] == rows_t[:top]).all() and np.abs(vals_r - vals_t).max() <= 1e-12
    for h in (rows_db, db):
        h.rescore([1.0, 0.7])
    assert np.abs(rows_db.scores() - db.scores()).max() <= 1e-12
    print("cfg1_10k as float16: %d of %d ranks settled" % (k, sc_r.size))
    rows_db.close()
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


ROUND_FIELDS = ("avg", "n_e", "scores", "match_rows", "near_rows")


def _same_result(a, b, fields=ROUND_FIELDS):
    return all(same_bits(getattr(a, f), getattr(b, f)) for f in fields) and a.near_argmax == b.near_argmax


@pytest.mark.parametrize("masked", [False, True])
def test_rounds_on_tiled16_against_the_row_major_twin(vqa, masked):
    """5 001 clips x 2 x 3: query_round (<= 1e-12, equal partitions: the bands are placed so that no score of either handle lies within
    2e-12 of an edge, which is asserted), query_round_batch and query_round_batch_sets (sets of tile_view_rows, an empty set and a
    whole-database member) with ``==`` on every field, and the calls on the round's averages -- fit, rescore, update, top-k -- ``==``
    the twin's: their inputs are identical bits."""
    n, s, e, q = 5_001, 2, 3, 7
    rng = np.random.default_rng(77)
    present = _mask(n, s, e) if masked else None
    plain = vqa.FeatureDB.synthetic(n, s, e, D, seed=41, scales=SCALES, dtype=F16)
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=41, scales=SCALES, dtype=F16)
    for h in (plain, db):
        h.set_present(present)
    db.set_layout("tiled16")
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
    near = np.sort(np.array(r_r.scores)[np.array(r_r.near_rows)])
    assert near[-1] - near[-2] > 2e-12 and r_r.near_argmax == r_t.near_argmax
    want = np_select(np.array(r_t.scores), th, lower)
    assert (np.array(r_t.match_rows) == want[0]).all() and (np.array(r_t.near_rows) == want[1]).all() and r_t.near_argmax == want[2]
    # batched rounds: the MFMA sequence of the rows, so the same bits everywhere
    targets = rng.standard_normal((q, s, e, D)) / D
    targets[0] = t
    weights = 0.5 + rng.random((q, s))
    ref = plain.query_round_batch(targets, weights, None)
    bands = np.array([np.quantile(ref[i].scores, [0.97, 0.90]) for i in range(q)])
    sets = {"a": tile_view_rows(n, 3), "b": tile_view_rows(n, 4)[::2], "none": np.zeros(0, dtype=np.int64)}
    for h in (plain, db):
        for name, rows in sets.items():
            h.define_search_rows(name, rows)
    set_ids = ["a", "b", "none", None, "a", "b", "none"]
    v_r, v_t = (h.query_round_batch_sets(targets, weights, set_ids, bands) for h in (plain, db))
    assert all(_same_result(a, b) for a, b in zip(v_r, v_t))
    b_r, b_t = plain.query_round_batch(targets, weights, bands), db.query_round_batch(targets, weights, bands)
    assert len(b_t) == q and all(_same_result(a, b) for a, b in zip(b_r, b_t))
    assert all(len(r.match_rows) > 0 and len(r.near_rows) > 0 for r in b_t)
    for i, sid in enumerate(set_ids):
        rows = np.arange(n) if sid is None else sets[sid]
        assert v_t[i].scores.shape == (rows.size,) and same_bits(v_t[i].scores, b_t[i].scores[rows]) and same_bits(v_t[i].avg, b_t[i].avg[rows])
    # the calls on the last batched round (the whole-database one above), the same arguments to both handles
    G, T = 9, 7
    cand, ths = np.stack([np.ones(G), np.linspace(0.5, 1.5, G)], axis=1), np.linspace(0.6, 0.9, T)
    lab = np.array([0, 7, 21, 40, 333, 4_999], dtype=np.int64)
    y = np.array([1.0, 0.0, 1.0, 0.0, 1.0, 0.0])

    def calls(h):
        fit = h.batch_round_fit([0, 2], [lab, lab[:3]], [y, y[:3]], [cand] * 2, [ths] * 2, [0.3] * 2)
        upd = h.batch_round_update([0, 3], [lab, lab[:4]], [y, y[:4]], [cand] * 2, [ths] * 2, [0.3] * 2, [1, 1], 1e-9, [0.35, 0.35], [None, None],
                                   want_surface=True)
        res = h.batch_round_rescore([1, 5], weights[[5, 1]], bands[[1, 5]])
        top = h.batch_round_topk(50)
        return fit, upd, res, top
    (fit_r, upd_r, res_r, top_r), (fit_t, upd_t, res_t, top_t) = calls(plain), calls(db)
    assert len(fit_t) == 2 and all(same_bits(np.array(a), np.array(b)) for a, b in zip(fit_r, fit_t))
    assert len(upd_t) == 2 and all(_same_result(a, b, ("scores", "match_rows", "near_rows", "surface")) for a, b in zip(upd_r, upd_t))
    assert all((float(a.w), float(a.threshold), float(a.lowest), a.iw, a.it, a.on_rim, a.fell_back) ==
               (float(b.w), float(b.threshold), float(b.lowest), b.iw, b.it, b.on_rim, b.fell_back) and tuple(a.band) == tuple(b.band)
               for a, b in zip(upd_r, upd_t))
    assert len(res_t) == 2 and all(_same_result(a, b, ("scores", "match_rows", "near_rows")) for a, b in zip(res_r, res_t))
    assert len(top_t) == q and all(same_bits(ra, rb) and same_bits(va, vb) for (ra, va), (rb, vb) in zip(top_r, top_t))
    plain.close()
    db.close()


def test_batch_targets_on_tiled16(vqa):
    """vq_db_batch_targets reads its rows through the gather of the layout: the targets of a tiled16 handle are the twin's bits."""
    n, s, e = 300, 2, 3
    plain = vqa.FeatureDB.synthetic(n, s, e, D, seed=43, scales=SCALES, dtype=F16)
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=43, scales=SCALES, dtype=F16)
    db.set_layout("tiled16")
    args = ([([3, 17, 31, 299], [100, 101, 250])], [[([0, 1, 2, 3], [0, 1]), ([1, 3], [2])]], [0.3])
    out_r, out_t = plain.batch_targets(*args), db.batch_targets(*args)
    assert len(out_r) == len(out_t) == 1 and out_t[0].shape == (s, e, D)
    assert np.isfinite(out_t[0]).all() and same_bits(out_r[0], out_t[0])
    plain.close()
    db.close()


def test_generate_on_a_tiled16_handle(vqa):
    """vq_db_generate writes rows; a tiled16 handle gets its layout back: the rows of another seed read back as a fresh database of
    that seed holds them, and the pass gives that database's bits."""
    import ctypes as C
    n, s, e = 53, 2, 2
    fresh = vqa.FeatureDB.synthetic(n, s, e, D, seed=9, scales=SCALES, dtype=F16)
    db = vqa.FeatureDB.synthetic(n, s, e, D, seed=8, scales=SCALES, dtype=F16)
    db.set_layout("tiled16")
    sc = np.ascontiguousarray(SCALES, dtype=np.float32)
    vqa._lib.call("vq_db_generate", db._h, C.c_uint64(9), 0, sc.ctypes.data_as(C.POINTER(C.c_float)))
    assert db.layout == "tiled16"
    every = np.arange(n)
    assert same_bits(db.read_rows(every), fresh.read_rows(every))
    assert same_bits(fresh.read_rows(every), so.synth_features(9, 0, n, s, e, D, SCALES).astype(F16))
    tg = np.random.default_rng(1).standard_normal((3, s, e, D)) / D
    assert (db.scan_batch(tg, np.ones((3, s))) == fresh.scan_batch(tg, np.ones((3, s)))).all()
    fresh.close()
    db.close()


def test_tiled16_is_refused_where_it_cannot_hold(vqa):
    """Each storage type has one tiled layout: "tiled16" on float32 / float64 and "tiled" / "tiled64" on float16 are VQ_E_UNSUPPORTED
    (-5), as are shapes without a tiled scan kernel; a block whose address was handed out is VQ_E_STATE (-4).  The handle works after
    each, and ``layouts`` names what each handle takes."""
    rng = np.random.default_rng(8)

    def works(db):
        tg = rng.standard_normal((2, db.S, db.E, db.D)) / db.D
        assert np.isfinite(db.scan_batch(tg, np.ones((2, db.S)))).all() and db.layout == "rows"
    for layout, kw, layouts in (("tiled16", {"dtype": np.float32}, ("rows", "tiled")), ("tiled16", {"dtype": np.float64}, ("rows", "tiled64")),
                                ("tiled", {}, ("rows", "tiled16")), ("tiled64", {}, ("rows", "tiled16")),
                                ("tiled16", {"dim": 256}, ("rows",)), ("tiled16", {"n_streams": 3}, ("rows",))):
        args = dict(n=200, n_streams=2, n_splits=2, dim=1024, dtype=F16)
        args.update(kw)
        db = vqa.FeatureDB.synthetic(args["n"], args["n_streams"], args["n_splits"], args["dim"], seed=3, scales=(2.0, 1.0, 1.0)[:args["n_streams"]],
                                     dtype=args["dtype"])
        with pytest.raises(vqa.VqError) as ei:
            db.set_layout(layout)
        assert ei.value.code == -5, (layout, kw)
        assert db.layouts == layouts and db.layouts[0] == "rows", (layout, kw, db.layouts)
        works(db)
        db.close()
    db = vqa.FeatureDB.synthetic(200, 2, 2, 1024, seed=31, scales=(2.0, 1.0), dtype=F16)
    assert db.layouts == ("rows", "tiled16") and db.tiled_layout is None
    db.feats_devptr()                                                  # from here on others may write the rows
    with pytest.raises(vqa.VqError) as ei:
        db.set_layout("tiled16")
    assert ei.value.code == -4
    works(db)
    with pytest.raises(KeyError):
        db.set_layout("tiled128")                                      # a name that is no layout never reaches the library
    works(db)
    db.close()


def test_csv_tree_into_tiled16(vqa, tmp_path):
    """from_csv_tree(layout="tiled16", dtype=float16): the values land in their tiles; read_rows equals the "rows" load bit for bit."""
    from video_query_algorithms_amd.tsn import feature_csv
    rng = np.random.default_rng(16)
    nclips = 37                                                        # two whole tiles and a ragged one
    feats = {m: (rng.random((nclips, 25, 1024)).astype(np.float32) * np.float32(2.0)).astype(np.float64).mean(axis=1) for m in feature_csv.STREAM_MODES}
    names = ["clip_%04d" % (i + 1) for i in range(nclips)]
    for split in (1, 2):
        feature_csv.write_features(str(tmp_path / "features"), "video_a", "/a/video_a.mp4", "UCF101_split%d" % split, "global_pool", names,
                                   feats, {m: m + ".caffemodel" for m in feature_csv.STREAM_MODES})
    rows_db = vqa.FeatureDB.from_csv_tree(str(tmp_path / "features"), dtype=F16)
    tiled = vqa.FeatureDB.from_csv_tree(str(tmp_path / "features"), dtype=F16, layout="tiled16")
    assert tiled.layout == "tiled16" and rows_db.layout == "rows" and (tiled.n, tiled.S, tiled.E, tiled.D) == (nclips, 2, 2, 1024)
    got, want = tiled.read_rows(np.arange(nclips)), rows_db.read_rows(np.arange(nclips))
    assert got.dtype == F16 and same_bits(got, want)
    for si, m in enumerate(feature_csv.STREAM_MODES):
        for ei in range(2):
            assert same_bits(got[:, si, ei], feats[m].astype(F16))      # the decimal text is the float64 mean: rounded once
    rows_db.close()
    tiled.close()
