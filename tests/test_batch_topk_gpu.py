"""GPU: the k best clips of every query of a batched round in one call (include/vq_amd_round_topk.h, FeatureDB.batch_round_topk).

The oracle is ``np_topk`` (tests/_search_set_cases.py) applied to the scores THE SAME ROUND copied back, so every comparison is exact:
``array_equal`` on the positions, ``same_bits`` on the values.  D = 256, S = 2, E = 1 and fp32 storage unless a case says otherwise.

One deviation from the plan of the cases: a score is 1 - sqrt(...) (ticket.py:172-180) and cannot exceed 1 whatever the target is scaled
by, so the "values above 1" of the sign case are PLANTED: the test overwrites the round's scores on the device (the array
vq_db_batch_scores_devptr names) with values of both signs, both zeros, infinities, NaNs, subnormals and values above 1, and ranks
those."""
import ctypes as C

import numpy as np
import pytest

from _search_set_cases import np_topk, presence_mask, same_bits, tie_ks, view_lists

pytestmark = pytest.mark.gpu
S, E, D = 2, 1, 256
SIZES = (1, 2, 2047, 2048, 2049, 16383, 16384, 16385, 40_001)       # the chunk of the selection kernels, kTopkSmallN +- 1, a long ragged piece
N_MAX = max(SIZES)
VQ_E_INVALID, VQ_E_STATE = -1, -4


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


_CACHE = {}


def features(n, d=D):
    """signed rows (similarities of both signs); the first n of one array per width, so every size shares its clips"""
    if d not in _CACHE:
        _CACHE[d] = np.random.default_rng(7).standard_normal((N_MAX if d == D else 2100, S, E, d), dtype=np.float32)
    return _CACHE[d][:n]


def targets(x, q, scale=None):
    """q targets: rows of x scaled as target_clip.py:311-313 does, times ``scale[i]``"""
    rows = (np.arange(q) * 37 + 1) % x.shape[0]
    t = np.stack([x[r].astype(np.float64) / np.maximum((x[r].astype(np.float64) ** 2).sum(axis=-1, keepdims=True), 1e-30) for r in rows])
    if scale is not None:
        t = t * np.asarray(scale, dtype=np.float64).reshape(-1, 1, 1, 1)
    return t


def weights(q):
    return np.stack([[1.0, 0.6 + 0.1 * i] for i in range(q)])


def cap_of(db):
    cap = db.batch_topk_cap()
    assert cap == 4096
    return cap


def k_list(m, q, cap):
    """a different k per query out of {1, 2, 20, 1024, 1025, cap, M, M + 5}; never one whose min(k, M) exceeds the cap"""
    ks = [k for k in (1, 2, 20, 1024, 1025, cap, m, m + 5) if min(k, m) <= cap]
    return [ks[i % len(ks)] for i in range(q)]


def check(db, scores, ks, queries=None, got=None):
    """batch_round_topk against np_topk of ``scores[q]`` (query q's scores as copied back), exactly"""
    queries = list(range(len(scores))) if queries is None else list(queries)
    ks = [ks] * len(queries) if np.ndim(ks) == 0 else list(ks)
    got = db.batch_round_topk(ks, None if queries == list(range(len(scores))) else queries) if got is None else got
    assert len(got) == len(queries)
    for (rows, vals), q, k in zip(got, queries, ks):
        want_rows, want_vals = np_topk(scores[q], k)
        assert rows.dtype == np.int64 and vals.dtype == np.float64
        assert np.array_equal(rows, want_rows), (q, k, rows[:8], want_rows[:8])
        assert same_bits(np.array(vals), np.array(want_vals)), (q, k)
        assert len(rows) == min(k, int((~np.isnan(scores[q])).sum()))
    return got


@pytest.mark.parametrize("m", SIZES)
def test_sizes_at_every_cut(vqa, m):
    """Q = 16 with a different k per query, then Q = 1, on a database of M clips."""
    x = features(m)
    db = vqa.FeatureDB.from_arrays(x)
    cap = cap_of(db)
    r = db.query_round_batch(targets(x, 16), weights(16))
    check(db, [np.array(v.scores) for v in r], k_list(m, 16, cap))
    r = db.query_round_batch(targets(x, 1), weights(1))
    for k in sorted(set(k_list(m, 8, cap))):
        check(db, [np.array(r[0].scores)], [k])
    if m > cap:                                                          # nothing clamps this k: the library's refusal, and the round still ranks
        with pytest.raises(vqa.VqError) as ei:
            db.batch_round_topk(cap + 1)
        assert ei.value.code == VQ_E_INVALID
        check(db, [np.array(r[0].scores)], [cap])
    db.close()


@pytest.mark.parametrize("m", [3000, 20_000], ids=["short", "long"])
def test_ties_across_the_boundary_keep_the_first_positions(vqa, m):
    base = features(7)
    db = vqa.FeatureDB.from_arrays(np.ascontiguousarray(base[np.arange(m) % 7]))
    cap = cap_of(db)
    r = db.query_round_batch(targets(base, 3), weights(3))
    scores = [np.array(v.scores) for v in r]
    assert all(np.unique(s).size <= 7 for s in scores)
    for k in tie_ks(scores[0], cap):
        got = check(db, scores, [k, k, k])
        rows, vals = got[0]
        last = vals[-1]
        tied = np.flatnonzero(scores[0] == last)
        assert np.array_equal(np.sort(rows[vals == last]), tied[:int((vals == last).sum())])      # the FIRST positions of the run
    db.close()
    # every score equal
    same = vqa.FeatureDB.from_arrays(np.ascontiguousarray(np.broadcast_to(base[3], (m, S, E, D))))
    r = same.query_round_batch(targets(base, 2), weights(2))
    scores = [np.array(v.scores) for v in r]
    assert np.unique(scores[0]).size == 1
    for k in (1, m // 2 if m // 2 <= cap else 1500, min(m, cap)):
        got = check(same, scores, [k, k])
        assert np.array_equal(got[0][0], np.arange(k))
    same.close()


def batch_scores_tensor(vqa, db, q, n):
    import torch
    p, nq = C.c_void_p(), C.c_int32()
    vqa._lib.call("vq_db_batch_scores_devptr", db._h, C.byref(p), C.byref(nq))
    assert nq.value == q

    class _View:
        __cuda_array_interface__ = {"shape": (q, n), "typestr": "<f8", "data": (int(p.value), False), "version": 2}
    return torch.as_tensor(_View(), device=torch.device("cuda", db.device))


@pytest.mark.parametrize("m", [5000, 20_000], ids=["short", "long"])
def test_signs(vqa, m):
    """Targets scaled by factors of both signs spread the scores over negative values and (0, 1); then planted scores of every kind."""
    import torch
    x = features(m)
    db = vqa.FeatureDB.from_arrays(x)
    cap = cap_of(db)
    q = 6
    r = db.query_round_batch(targets(x, q, scale=[1.0, -1.0, 40.0, 0.02, -300.0, 3.0]), weights(q))
    scores = [np.array(v.scores) for v in r]
    assert any((s < 0).any() and ((s > 0) & (s < 1)).any() for s in scores)
    check(db, scores, [20, 1025, cap, 1, 1024, 300])
    # planted: the snapshot's scores are whatever the device block holds
    rng = np.random.default_rng(3)
    planted = rng.standard_normal((q, m)) * np.array([1.0, 1e-3, 50.0, 1e300, 1e-310, 2.0]).reshape(q, 1)
    planted[0] = -np.abs(planted[0])                                      # the zeros planted next are its best scores
    planted[0, rng.integers(0, m, 400)] = 0.0
    planted[0, rng.integers(0, m, 400)] = -0.0
    planted[1, rng.integers(0, m, 50)] = np.inf
    planted[1, rng.integers(0, m, 50)] = -np.inf
    planted[2, rng.integers(0, m, m // 3)] = np.nan
    planted[2, rng.integers(0, m, 30)] = -np.nan
    planted[3] = np.round(planted[3] / 1e300 * 4) / 4 + 1.5                # few distinct values, most above 1
    planted[5] = np.abs(planted[5]) + 1.0                                 # all above 1
    dev = batch_scores_tensor(vqa, db, q, m)
    dev.copy_(torch.from_numpy(planted))
    torch.cuda.synchronize()
    back = dev.cpu().numpy()
    assert same_bits(back, planted)
    for ks in ([20] * q, [1025, 2, cap, 1024, 777, min(m, cap)], [min(m, cap)] * q):
        check(db, list(back), ks)
    got = db.batch_round_topk(min(m, cap), [0])[0]
    zeros = got[0][got[1] == 0.0]
    assert zeros.size > 1 and (np.diff(zeros) > 0).all()                  # -0 and +0 tie: position order
    db.close()


@pytest.mark.parametrize("m", [1200, 3000, 20_000], ids=["short", "short-db-long-k", "long"])
def test_nan_rows_are_absent(vqa, m):
    x = features(m)
    db = vqa.FeatureDB.from_arrays(x, present=presence_mask(m, S, E))
    cap = cap_of(db)
    r = db.query_round_batch(targets(x, 4), weights(4))
    scores = [np.array(v.scores) for v in r]
    finite = int((~np.isnan(scores[0])).sum())
    assert 0 < finite < m and np.isnan(scores[0][1]) and np.isnan(scores[0][m - 1])
    ks = [min(m, cap), 20, min(finite + 1, cap), min(finite, cap)]          # the first exceeds the non-NaN count when M <= cap
    got = check(db, scores, ks)
    if m <= cap:
        assert len(got[0][0]) == finite < ks[0]
    for rows, _vals in got:
        assert not np.isnan(scores[0][rows]).any()
    db.close()


SET_ORDER = ["empty", "first", "last", "every_second", "runs", "random_half", None]


@pytest.mark.parametrize("n,d,layout", [(20_000, D, "rows"), (40_001, D, "rows"), (2100, 1024, "tiled")], ids=["rows", "rows-long-sets", "tiled"])
def test_view_rounds_rank_positions_of_each_set(vqa, n, d, layout):
    x = features(n, d)
    db = vqa.FeatureDB.from_arrays(x)
    if layout == "tiled":
        db.set_layout("tiled")
    cap = cap_of(db)
    lists = view_lists(n)
    for name in SET_ORDER:
        if name is not None:
            db.define_search_rows(name, lists[name])
    q = len(SET_ORDER)
    r = db.query_round_batch_sets(targets(x, q), weights(q), SET_ORDER)
    scores = [np.array(v.scores) for v in r]
    sizes = [0, 1, 1, lists["every_second"].size, lists["runs"].size, lists["random_half"].size, n]
    assert [s.size for s in scores] == sizes
    got = check(db, scores, [5, 5, 1, 1025, cap, 20, cap])
    assert len(got[0][0]) == 0 and len(got[1][0]) == 1 and got[1][0][0] == 0
    for (rows, _v), size in zip(got, sizes):
        assert rows.size == 0 or (0 <= rows.min() and rows.max() < size)          # positions in the set, not database rows
    # against the whole-database round: the same clips, through the set's rows
    whole = db.query_round_batch(targets(x, q), weights(q))
    for i, name in enumerate(SET_ORDER[1:-1], start=1):
        assert same_bits(np.array(whole[i].scores)[lists[name]], scores[i])
    check(db, [np.array(v.scores) for v in whole], [20] * q)
    db.close()


@pytest.mark.parametrize("n,views", [(3000, False), (20_000, False), (20_000, True)], ids=["short", "long", "long-views"])
def test_after_a_rescore_the_masked_queries_rank_under_their_new_scores(vqa, n, views):
    x = features(n)
    db = vqa.FeatureDB.from_arrays(x)
    q = 5
    sets = ["a", None, "b", "a", None]
    if views:
        db.define_search_rows("a", np.arange(3, n, 3))
        db.define_search_rows("b", np.arange(100, n - 50))
        r = db.query_round_batch_sets(targets(x, q), weights(q), sets)
    else:
        r = db.query_round_batch(targets(x, q), weights(q))
    scores = [np.array(v.scores) for v in r]
    check(db, scores, [50] * q)
    again = db.batch_round_rescore([1, 3], np.array([[1.0, 2.5], [0.3, 1.0]]), np.array([[0.8, 0.7], [0.8, 0.7]]))
    for i, res in zip((1, 3), again):
        assert not same_bits(np.array(res.scores), scores[i])
        scores[i] = np.array(res.scores)
    check(db, scores, [50, 1025, 20, 1, 4096])
    check(db, scores, [7, 7], queries=[3, 0])
    db.close()


@pytest.mark.parametrize("n,views", [(3000, False), (20_000, True)], ids=["whole", "views"])
def test_without_scores_copied_back(vqa, n, views):
    x = features(n)
    db = vqa.FeatureDB.from_arrays(x)
    q = 4
    sets = ["a", None, "a", None]
    if views:
        db.define_search_rows("a", np.arange(1, n, 2))

    def run(want_scores):
        if views:
            return db.query_round_batch_sets(targets(x, q), weights(q), sets, np.array([[0.5, 0.2]] * q), want_scores=want_scores)
        return db.query_round_batch(targets(x, q), weights(q), np.array([[0.5, 0.2]] * q), want_scores=want_scores)
    bare = run(False)
    assert all(v.scores is None for v in bare) and all(v.avg is not None and v.match_rows is not None for v in bare)
    got = [(np.array(rows), np.array(vals)) for rows, vals in db.batch_round_topk([20, 1025, 1, 300])]
    full = run(True)
    assert all(np.array_equal(a.match_rows, b.match_rows) and np.array_equal(a.near_rows, b.near_rows) for a, b in zip(bare, full))
    check(db, [np.array(v.scores) for v in full], [20, 1025, 1, 300], got=got)
    check(db, [np.array(v.scores) for v in full], [20, 1025, 1, 300])
    db.close()


def fetch_lists(vqa, db, q, nm, nn):
    m, k = np.empty(max(nm, 1), dtype=np.int64), np.empty(max(nn, 1), dtype=np.int64)
    vqa._lib.call("vq_db_batch_round_fetch", db._h, q, m.ctypes.data_as(C.c_void_p), nm, k.ctypes.data_as(C.c_void_p), nn)
    return m[:nm], k[:nn]


@pytest.mark.parametrize("n", [3000, 20_000], ids=["short", "long"])
def test_snapshot_and_handle_are_left_alone(vqa, n):
    """Two identical databases run the same one-query round and the same view round; one of them ranks in between."""
    x = features(n)
    q = 4
    sets = ["a", None, "b", None]
    bands = np.array([[0.2, -0.5]] * q)
    state = []
    for rank in (False, True):
        db = vqa.FeatureDB.from_arrays(x)
        db.define_search_rows("a", np.arange(2, n, 2))
        db.define_search_rows("b", np.arange(50, n - 50))
        db.use_search_set("a")
        db.set_query(targets(x, 1)[0])
        db.scan(weights=[1.0, 1.3])
        before = (db.scores(), db.topk(10), db.select(0.3, -0.2))
        r = db.query_round_batch_sets(targets(x, q), weights(q), sets, bands)
        lists = [(np.array(v.match_rows), np.array(v.near_rows)) for v in r]
        assert max(len(m) + len(k) for m, k in lists) > 2048                          # lists beyond the prefix: the full lists are used
        if rank:
            check(db, [np.array(v.scores) for v in r], [20, 4096, 1025, 1])
            check(db, [np.array(v.scores) for v in r], [4096], queries=[2])
        view, covered = C.c_int32(), C.c_int64()
        vqa._lib.call("vq_db_rows_active", db._h, C.byref(view), C.byref(covered))
        assert db.search_set_in_use == "a" and view.value == db.search_set_view("a").token and covered.value == db.search_set_view("a").n
        for i, (m, k) in enumerate(lists):
            fm, fk = fetch_lists(vqa, db, i, len(m), len(k))
            assert np.array_equal(fm, m) and np.array_equal(fk, k)
        after = (db.scores(), db.topk(10), db.select(0.3, -0.2))
        assert same_bits(before[0], after[0])
        assert np.array_equal(before[1][0], after[1][0]) and same_bits(before[1][1], after[1][1])
        assert all(np.array_equal(a, b) for a, b in zip(before[2][:2], after[2][:2])) and before[2][2] == after[2][2]
        hp = vqa.Hyperparameter({"rgb": 1.0, "warped_optical_flow": 1.5})
        cand = np.zeros((len(hp.weight_grid), S))
        cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
        ths = np.asarray(hp.threshold_grid, dtype=np.float64)
        rows = [np.arange(0, 40, dtype=np.int64) * 7, np.arange(0, 25, dtype=np.int64) * 11]
        labels = [(np.arange(40) % 3 == 0).astype(np.float64), (np.arange(25) % 2 == 0).astype(np.float64)]
        surfaces = [np.array(s) for s in db.batch_round_fit([0, 3], rows, labels, [cand] * 2, [ths] * 2, [0.3, 0.3])]
        if rank:
            check(db, [np.array(v.scores) for v in r], [33] * q)
        again = db.batch_round_rescore([1, 2], np.array([[1.0, 2.0], [0.4, 1.0]]), np.array([[0.25, -0.4], [0.25, -0.4]]))
        state.append((before, [np.array(v.scores) for v in r], lists, surfaces,
                      [(np.array(v.scores), np.array(v.match_rows), np.array(v.near_rows), v.near_argmax) for v in again]))
        if rank:
            new = [np.array(v.scores) for v in r]
            new[1], new[2] = state[-1][4][0][0], state[-1][4][1][0]
            check(db, new, [20] * q)
        db.close()
    plain, ranked = state
    assert same_bits(plain[0][0], ranked[0][0])
    assert all(same_bits(a, b) for a, b in zip(plain[1], ranked[1]))
    assert all(same_bits(a, b) for a, b in zip(plain[3], ranked[3]))
    for a, b in zip(plain[4], ranked[4]):
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def raw_call(vqa, db, q, k_max, ks, sentinel=0xA5, short_by=0):
    """the C call on a block filled with a sentinel: (rc, count, rows, vals, k)"""
    off = (C.c_int64 * 6)()
    vqa._lib.call("vq_db_batch_topk_layout", db._h, q, k_max, off)
    off = [int(v) for v in off]
    blk = db.blocks.take("topk", off[4])
    raw = blk.bytes()
    raw[...] = sentinel
    raw[off[0]:off[0] + 8 * q].view(np.int64)[...] = ks
    rc = vqa.load_library().vq_db_batch_round_topk(db._h, q, k_max, C.c_void_p(blk.ptr), off[4] - short_by if short_by else blk.nbytes)
    piece = lambda i, dtype, shape: raw[off[i]:off[i] + int(np.prod(shape)) * 8].view(dtype).reshape(shape)
    return rc, piece(1, np.int64, (q,)), piece(2, np.int64, (q, k_max)), piece(3, np.float64, (q, k_max)), raw


@pytest.mark.parametrize("n", [3000, 20_000], ids=["short", "long"])
def test_skipped_slots_keep_what_the_caller_left(vqa, n):
    x = features(n)
    db = vqa.FeatureDB.from_arrays(x)
    q = 6
    r = db.query_round_batch(targets(x, q), weights(q))
    scores = [np.array(v.scores) for v in r]
    ks = [0, 30, 40, 0, 1100, 0]
    rc, count, rows, vals, _raw = raw_call(vqa, db, q, 1100, ks)
    assert rc == 0
    mark = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]
    for i, k in enumerate(ks):
        if k == 0:
            assert count[i] == mark and (rows[i] == mark).all() and (vals[i].view(np.int64) == mark).all()
        else:
            want_rows, want_vals = np_topk(scores[i], k)
            assert count[i] == k and np.array_equal(rows[i, :k], want_rows) and same_bits(np.array(vals[i, :k]), want_vals)
    # a query of the round beyond n_queries is simply not served; every k zero is a call that launches nothing
    rc, count, rows, _vals, _raw = raw_call(vqa, db, 2, 8, [0, 8])
    assert rc == 0 and count[0] == mark and count[1] == 8 and np.array_equal(rows[1], np_topk(scores[1], 8)[0])
    rc, count, _rows, _vals, _raw = raw_call(vqa, db, 3, 8, [0, 0, 0])
    assert rc == 0 and (count == mark).all()
    db.close()


def test_errors_leave_the_snapshot_usable(vqa):
    n = 3000
    x = features(n)
    db = vqa.FeatureDB.from_arrays(x)
    with pytest.raises(vqa.VqError) as ei:                               # no round yet
        db.batch_round_topk(5)
    assert ei.value.code == VQ_E_STATE
    assert raw_call(vqa, db, 2, 8, [3, 3])[0] == VQ_E_STATE
    r = db.query_round_batch(targets(x, 3), weights(3))
    scores = [np.array(v.scores) for v in r]
    check(db, scores, [5, 6, 7])
    with pytest.raises(vqa.VqError) as ei:                               # a slot the round did not have
        db.batch_round_topk([5], queries=[4])
    assert ei.value.code == VQ_E_STATE
    check(db, scores, [5, 6, 7])
    assert raw_call(vqa, db, 4, 8, [3, 3, 3, 3])[0] == VQ_E_STATE
    check(db, scores, [5, 6, 7])
    assert raw_call(vqa, db, 4, 8, [3, 3, 3, 0])[0] == 0                  # ... but a skipped one is no error
    cap = cap_of(db)
    for ks, k_max, short_by in (([3, 9, 3], 8, 0), ([3, -1, 3], 8, 0), ([3, 3, 3], 8, 64), ([3, 3, 3], 8, 1)):
        assert raw_call(vqa, db, 3, k_max, ks, short_by=short_by)[0] == VQ_E_INVALID, (ks, k_max, short_by)
        check(db, scores, [5, 6, 7])
    with pytest.raises(vqa.VqError) as ei:                               # above the cap: the library's refusal, from the layout call on
        raw_call(vqa, db, 3, cap + 1, [3, 3, 3])
    assert ei.value.code == VQ_E_INVALID
    block = db.blocks.take("topk", 64)
    assert vqa.load_library().vq_db_batch_round_topk(db._h, 3, cap + 1, C.c_void_p(block.ptr), block.nbytes) == VQ_E_INVALID
    check(db, scores, [5, 6, 7])
    with pytest.raises(ValueError):
        db.batch_round_topk([1, 2])
    check(db, scores, [n, 1, 20])                                        # min(k, M) = 3000 <= cap
    db.close()


@pytest.mark.parametrize("dtype", [np.float16, np.float64], ids=["f16", "f64"])
@pytest.mark.parametrize("m", [2049, 16385])
def test_storage_types(vqa, dtype, m):
    x = (features(m) * 0.25).astype(dtype)
    db = vqa.FeatureDB.from_arrays(x, dtype=dtype)
    cap = cap_of(db)
    r = db.query_round_batch(targets(x.astype(np.float32), 8), weights(8))
    check(db, [np.array(v.scores) for v in r], k_list(m, 8, cap))
    db.close()
