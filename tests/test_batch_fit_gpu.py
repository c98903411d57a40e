"""GPU: the weight fit and the re-weighting of a batched round's queries (include/vq_amd_round_fit.h, FeatureDB.batch_round_fit /
batch_round_rescore) against the one-query calls on a second, identical database that got the round's averaged similarities through
write_avg: loss_surface / scores_grid, rescore + scores, select.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import sim_oracle as so
from _search_set_cases import host_loss_surface, same_bits

pytestmark = pytest.mark.gpu
BALLAST = 0.3
MEMBERS = (1, 3, 4)                       # of the five queries of a round: a gap, and the last slot in use
SMALL, BIG = (2000, 2, 3, 1024), (17_000, 2, 1, 256)      # one-workgroup selection | three passes (above kSelSmallN = 16384)
REFS = (11, 300, 777, 1203, 1650)


def blended(shape, seed):
    """so.cfg1_features-like rows where every reference clip has 80 relatives a x[ref] + (1 - a) x[clip], so that the scores against
    it fill the near band and the match band (the recipe of tests/test_batch_tickets_gpu.py); row 1500 is a copy of clip REFS[3]."""
    n, s, e, d = shape
    if shape == SMALL:
        x = so.cfg1_features(n=n, e=e, seed=21)
    else:
        x = np.abs(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)) * np.array([3.8, 1.2], dtype=np.float32).reshape(1, s, 1, 1)
    for k, ref in enumerate(REFS):
        rel = (ref + 3 + 5 * np.arange(80)) % n
        a = np.linspace(0.05, 0.98, 80, dtype=np.float32)[np.random.default_rng(k).permutation(80)].reshape(-1, 1, 1, 1)
        x[rel] = a * x[ref] + (1 - a) * x[rel]
    x[1500] = x[REFS[3]]
    return x


_CACHE = {}


def data(shape):
    if shape not in _CACHE:
        x = blended(shape, seed=5)
        t = np.stack([np.stack([[so.scale_feature(x[r, s, e].astype(np.float64)) for e in range(shape[2])] for s in range(shape[1])]) for r in REFS])
        _CACHE[shape] = (x, t)
    return _CACHE[shape]


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def grids(vqa, S):
    hp = vqa.Hyperparameter({"rgb": 1.0, "warped_optical_flow": 1.5})
    cand = np.zeros((len(hp.weight_grid), S))
    cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
    assert cand.shape[0] == 40 and hp.threshold_grid.shape == (31,)                           # the reference's 40 x 31
    return cand, np.asarray(hp.threshold_grid, dtype=np.float64)


def pair(vqa, shape, dtype=np.float32, layout="rows"):
    x, t = data(shape)
    out = []
    for _ in range(2):
        db = vqa.FeatureDB.from_arrays(x.astype(dtype), dtype=dtype)
        if layout == "tiled":
            db.set_layout("tiled")
        out.append(db)
    return out[0], out[1], t


W0 = np.array([[1.0, 1.5], [1.0, 0.8], [1.0, 2.0], [1.0, 1.1], [1.0, 0.6]])
BANDS0 = np.array([[0.8, 0.73]] * 5)
SETS = ["a", None, "empty", "b", "c"]                     # of the five queries of a view round


def define_sets(db, n):
    rows = np.arange(n, dtype=np.int64)
    db.define_search_rows("a", rows[3::7])
    db.define_search_rows("empty", rows[:0])
    db.define_search_rows("b", rows[100:n - 300])
    db.define_search_rows("c", rows[::2])


def run_round(db, t, views):
    return db.query_round_batch_sets(t, W0, SETS, BANDS0) if views else db.query_round_batch(t, W0, BANDS0)


def hand_over(ref, r, q, views):
    """``ref`` gets query q's averaged similarities of the round, under the query's search set"""
    if views:
        ref.use_search_set(SETS[q])
    ref.write_avg(np.array(r.avg), np.array(r.n_e))


def labels_for(m, counts, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, m_q, size=c).astype(np.int64), (rng.random(c) < 0.4).astype(np.float64)) for m_q, c in zip(m, counts)]


def check_fit(vqa, db, ref, results, views, counts):
    cand, ths = grids(vqa, db.S)
    lab = labels_for([results[q].scores.shape[0] for q in MEMBERS], counts)
    surfaces = db.batch_round_fit(list(MEMBERS), [l[0] for l in lab], [l[1] for l in lab], [cand] * 3, [ths] * 3, [BALLAST] * 3)
    for q, (rows, y), surface in zip(MEMBERS, lab, surfaces):
        hand_over(ref, results[q], q, views)
        assert surface.shape == (40, 31) and np.isfinite(surface).all()
        if len(rows) <= 4096:
            assert same_bits(surface, ref.loss_surface(cand, rows, y, ths, BALLAST)), (q, len(rows))
        assert same_bits(surface, host_loss_surface(ref.scores_grid(cand, rows), y, ths, BALLAST)), (q, len(rows))
    return lab, surfaces


@pytest.mark.parametrize("shape,dtype,layout,views,counts", [
    (SMALL, np.float32, "rows", False, (20, 1, 1500)), (SMALL, np.float32, "rows", True, (20, 1, 700)),
    (SMALL, np.float32, "tiled", False, (20, 1, 33)), (SMALL, np.float16, "rows", False, (20, 1, 33)),
    (BIG, np.float32, "rows", False, (20, 1, 4097)), (BIG, np.float32, "rows", True, (20, 1, 4097))],
    ids=["small", "small-views", "small-tiled", "small-f16", "big-4097", "big-views-4097"])
def test_fit_equals_the_one_query_loss_surface(vqa, shape, dtype, layout, views, counts):
    """Queries 1, 3 and 4 of a round of five, L = 20, 1 and a long list (4097: a second chunk of exactly one label): every surface has
    the bits of loss_surface (L <= 4096) and of the host route over scores_grid, on the same avg."""
    db, ref, t = pair(vqa, shape, dtype, layout)
    if views:
        define_sets(db, shape[0])
        define_sets(ref, shape[0])
    check_fit(vqa, db, ref, run_round(db, t, views), views, counts)
    db.close()
    ref.close()


def raw_fit(vqa, db, Q, G, T, entries, short=0):
    """vq_db_batch_round_fit on a block prefilled with 0xA5 bytes.  entries: {q: (rows, labels, w_grid [G,S], th [T], ballast)} ->
    (surface [Q,G,T] as the block holds it afterwards, the block's bytes)."""
    total = sum(len(e[0]) for e in entries.values())
    off = (C.c_int64 * 8)()
    vqa._lib.call("vq_db_batch_fit_layout", db._h, Q, G, T, total, off)
    off = [int(v) for v in off]
    blk = db.blocks.take("fit", off[7])
    raw = blk.bytes()
    raw[:off[7]] = 0xA5
    raw[off[3]:off[3] + 8 * Q].view(np.int64)[:] = 0
    at = 0
    for q in sorted(entries):
        rows, y, wg, th, ballast = entries[q]
        w = np.zeros((G, 8))
        w[:, :db.S] = wg
        raw[off[0] + q * G * 64:off[0] + (q + 1) * G * 64].view(np.float64)[:] = w.reshape(-1)
        raw[off[1] + q * T * 8:off[1] + (q + 1) * T * 8].view(np.float64)[:] = th
        raw[off[2] + q * 8:off[2] + q * 8 + 8].view(np.float64)[:] = ballast
        raw[off[3] + q * 8:off[3] + q * 8 + 8].view(np.int64)[:] = len(rows)
        raw[off[4] + at * 8:off[4] + (at + len(rows)) * 8].view(np.int64)[:] = rows
        raw[off[5] + at * 8:off[5] + (at + len(rows)) * 8].view(np.float64)[:] = y
        at += len(rows)
    vqa._lib.call("vq_db_batch_round_fit", db._h, Q, G, T, total, C.c_void_p(blk.ptr), off[7] - short)
    return raw[off[6]:off[6] + Q * G * T * 8].view(np.float64).reshape(Q, G, T), raw


def test_skipped_queries_are_not_written_and_the_snapshot_outlives_later_calls(vqa):
    """The cells of queries without labels keep the bytes the block came with; after an upload over some rows and a one-query round
    on the handle the fit and the re-weighting still work on the batched round's similarities."""
    db, ref, t = pair(vqa, SMALL)
    results = run_round(db, t, False)
    lab, surfaces = check_fit(vqa, db, ref, results, False, (20, 1, 300))
    cand, ths = grids(vqa, db.S)
    surface, _raw = raw_fit(vqa, db, 5, 40, 31, {q: (l[0], l[1], cand, ths, BALLAST) for q, l in zip(MEMBERS, lab)})
    for q in range(5):
        if q in MEMBERS:
            assert same_bits(surface[q], surfaces[MEMBERS.index(q)])
        else:
            assert (surface[q].view(np.uint8) == 0xA5).all()
    # later one-query work on the handle: other rows, another query, other scores
    x, _t = data(SMALL)
    db.upload(0, np.ascontiguousarray(x[500:520]))
    db.set_present(np.ones((SMALL[0], 2, 3), dtype=np.uint8))
    db.query_round(t[2], weights=np.array([1.0, 0.7]), select=(0.8, 0.7))
    again = db.batch_round_fit(list(MEMBERS), [l[0] for l in lab], [l[1] for l in lab], [cand] * 3, [ths] * 3, [BALLAST] * 3)
    assert all(same_bits(a, b) for a, b in zip(again, surfaces))
    hand_over(ref, results[3], 3, False)
    ref.rescore([1.0, 0.9])
    got = db.batch_round_rescore([3], np.array([[1.0, 0.9]]), np.array([[0.8, 0.7]]))[0]
    assert same_bits(got.scores, ref.scores())
    m, k, am = ref.select(0.8, 0.7)
    assert (got.match_rows == m).all() and (got.near_rows == k).all() and got.near_argmax == am and got.avg is results[3].avg
    db.close()
    ref.close()


def fetch(vqa, db, q, nm, nn):
    m, k = np.empty(nm, dtype=np.int64), np.empty(nn, dtype=np.int64)
    vqa._lib.call("vq_db_batch_round_fetch", db._h, q, m.ctypes.data_as(C.c_void_p) if nm else None, nm, k.ctypes.data_as(C.c_void_p) if nn else None, nn)
    return m, k


def device_scores(vqa, db, Q, n):
    ptr, nq = C.c_void_p(), C.c_int32()
    vqa._lib.call("vq_db_batch_scores_devptr", db._h, C.byref(ptr), C.byref(nq))
    out = np.empty((Q, n), dtype=np.float64)
    vqa._lib.call("vq_dev_read", out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 0)
    return out


W1 = np.array([[1.0, 0.9], [1.0, 2.2], [1.0, 1.3], [1.0, 0.55], [1.0, 1.7]])


@pytest.mark.parametrize("shape,views", [(SMALL, False), (SMALL, True), (BIG, False), (BIG, True)], ids=["small", "small-views", "big", "big-views"])
@pytest.mark.parametrize("mask", [(0,), (1, 3, 4), (0, 1, 2, 3, 4)], ids=["m0", "m134", "all"])
def test_rescore_equals_the_one_query_rescore_and_select(vqa, shape, views, mask):
    """The masked queries get rescore + scores and select of the reference database on the same avg, under a band with empty lists, one
    with lists inside the 1024-row prefix and one whose match list is longer (the fetch path); the others keep scores, lists and
    counts of the round, in what the call returns, in vq_db_batch_round_fetch and in the device's score array."""
    db, ref, t = pair(vqa, shape)
    n = shape[0]
    if views:
        define_sets(db, n)
        define_sets(ref, n)
    results = run_round(db, t, views)
    before = [(np.array(r.scores), np.array(r.match_rows), np.array(r.near_rows), r.near_argmax) for r in results]
    want, bands = {}, []
    for i, q in enumerate(mask):
        if results[q].scores.shape[0] == 0:                                                    # the empty search set: nothing to hand over
            bands.append((0.8, 0.7))
            want[q] = (np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), -1)
            continue
        hand_over(ref, results[q], q, views)
        ref.rescore(W1[q])
        sc = ref.scores()
        if i % 3 == 0:
            band = (float(np.quantile(sc, 0.8)) if n > 16384 else float(np.quantile(sc, 0.99)), float(np.quantile(sc, 0.75)))      # big: > 1024 matches
        elif i % 3 == 1:
            band = (2.0, 1.5)                                                                  # nothing matches, nothing is near
        else:
            band = (float(np.quantile(sc, 0.995)), float(np.quantile(sc, 0.97)))
        bands.append(band)
        want[q] = (sc,) + tuple(ref.select(*band))
    got = db.batch_round_rescore(list(mask), W1[list(mask)], np.array(bands))
    for q, r in zip(mask, got):
        sc, m, k, am = want[q]
        assert same_bits(r.scores, sc), q
        assert np.array_equal(r.match_rows, m) and np.array_equal(r.near_rows, k) and r.near_argmax == am, q
        fm, fk = fetch(vqa, db, q, len(m), len(k))
        assert np.array_equal(fm, m) and np.array_equal(fk, k)
        assert r.avg is results[q].avg and r.n_e is results[q].n_e
    if n > 16384 and not views:
        assert len(want[mask[0]][1]) > 1024                                                    # the fetch path ran
    assert len(want[mask[0]][1]) > 0 and len(want[mask[0]][2]) > 1                             # a real band
    for q in range(5):
        if q not in mask:
            sc, m, k, am = before[q]
            fm, fk = fetch(vqa, db, q, len(m), len(k))
            assert np.array_equal(fm, m) and np.array_equal(fk, k), q
            assert same_bits(results[q].scores, sc)                                            # the round's own arrays were not touched
    if not views:
        dev = device_scores(vqa, db, 5, n)
        for q in range(5):
            assert same_bits(dev[q], want[q][0] if q in mask else before[q][0]), q
    db.close()
    ref.close()


def test_rescore_leaves_the_block_of_unmasked_queries_alone_and_ties_go_to_the_first_row(vqa):
    """The library call on a block prefilled with 0xA5: only the masked queries' scores, results and prefixes are written.  Rows 1203
    and 1500 hold the clip query 3 is made from: both have the largest near score and near_argmax is row 1203, the first."""
    db, ref, t = pair(vqa, SMALL)
    results = run_round(db, t, False)
    Q, off = db._bround_last.Q, db._bround_last.off
    hand_over(ref, results[3], 3, False)
    ref.rescore(W1[3])
    sc = ref.scores()
    assert sc[1203] == sc[1500] == sc.max()
    th = float(np.nextafter(sc[1203], 2.0))
    band = (th, float(np.sort(sc)[-31]))                                                      # the 31 best clips are near, none matches
    m, k, am = ref.select(*band)
    assert am == 1203 and 1500 in k and len(m) == 0 and 31 <= len(k) < 40
    blk = db.blocks.take("fit", off[9])
    raw = blk.bytes()
    raw[:off[9]] = 0xA5
    wv = raw[off[1]:off[1] + Q * 64].view(np.float64).reshape(Q, 8)
    wv[3] = 0.0
    wv[3, :2] = W1[3]
    raw[off[2]:off[2] + Q * 16].view(np.float64).reshape(Q, 2)[3] = band
    vqa._lib.call("vq_db_batch_round_rescore", db._h, 1 << 3, C.c_void_p(blk.ptr), off[9], 6)
    n, P = SMALL[0], off[10]
    scores = raw[off[5]:off[5] + Q * n * 8].view(np.float64).reshape(Q, n)
    res = raw[off[6]:off[6] + Q * 32].view(np.int64).reshape(Q, 4)
    pre = [raw[off[p]:off[p] + Q * P * 8].view(np.int64).reshape(Q, P) for p in (7, 8)]
    assert same_bits(scores[3], sc) and res[3].tolist() == [len(m), len(k), 1203, 0]
    assert (pre[0][3, :len(m)] == m).all() and (pre[1][3, :len(k)] == k).all()
    for q in (0, 1, 2, 4):
        assert all((a[q].view(np.uint8) == 0xA5).all() for a in (scores, res, pre[0], pre[1])), q
    assert (raw[off[3]:off[5]] == 0xA5).all() and (raw[:off[1]] == 0xA5).all()                # n_e, avg and the queries: never written
    db.close()
    ref.close()


def test_refusals_are_argument_checks_and_leave_the_round_usable(vqa):
    db, ref, t = pair(vqa, SMALL)
    cand, ths = grids(vqa, db.S)
    rows, y = np.array([5, 9, 1999], dtype=np.int64), np.array([1.0, 0.0, 1.0])

    def refused(code, fn, *a, **kw):
        with pytest.raises(vqa.VqError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code, str(ei.value)
    # no batched round yet
    refused(-4, db.batch_round_fit, [0], [rows], [y], [cand], [ths], [BALLAST])
    refused(-4, db.batch_round_rescore, [0], W1[:1], BANDS0[:1])
    results = run_round(db, t, False)
    refused(-4, db.batch_round_fit, [5], [rows], [y], [cand], [ths], [BALLAST])              # a query the round did not have
    refused(-4, db.batch_round_rescore, [5], W1[:1], BANDS0[:1])
    refused(-1, db.batch_round_fit, [1], [np.array([5, 2000])], [y[:2]], [cand], [ths], [BALLAST])      # a row = M_q
    refused(-1, db.batch_round_fit, [1], [np.array([-1])], [y[:1]], [cand], [ths], [BALLAST])
    refused(-1, db.batch_round_fit, [1], [rows], [y], [np.ones((65, 2))], [ths], [BALLAST])  # G = 65
    refused(-1, db.batch_round_fit, [1], [rows], [y], [cand], [np.linspace(0.5, 1.0, 65)], [BALLAST])   # T = 65
    refused(-1, raw_fit, vqa, db, 5, 40, 31, {1: (rows, y, cand, ths, BALLAST)}, short=64)   # a short block
    off = db._bround_last.off
    blk = db.blocks.take("fit", off[9])
    lib = vqa.load_library()
    assert lib.vq_db_batch_round_rescore(db._h, 2, C.c_void_p(blk.ptr), off[9] - 64, 6) == -1           # a short block
    assert lib.vq_db_batch_round_rescore(db._h, 2, C.c_void_p(blk.ptr), off[9], 8) == -1                # an unknown flag
    assert lib.vq_db_batch_round_rescore(db._h, 0, C.c_void_p(blk.ptr), off[9], 6) == -1                # nobody
    # the round is still there, for both calls
    hand_over(ref, results[1], 1, False)
    surface = db.batch_round_fit([1], [rows], [y], [cand], [ths], [BALLAST])[0]
    assert same_bits(surface, ref.loss_surface(cand, rows, y, ths, BALLAST))
    ref.rescore(W1[1])
    got = db.batch_round_rescore([1], W1[1:2], BANDS0[:1])[0]
    m, k, am = ref.select(*BANDS0[0])
    assert same_bits(got.scores, ref.scores()) and (got.match_rows == m).all() and (got.near_rows == k).all() and got.near_argmax == am
    db.close()
    ref.close()
