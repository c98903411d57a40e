"""GPU: batched rounds with a search set per query (include/vq_amd_round_views.h, FeatureDB.query_round_batch_sets) -- one pass over the
union of the sets -- against query_round_batch on the same handle (bit for bit), the one-query round under use_search_set and
oracle/sim_oracle.py (<= 1e-12), and a numpy stable partition of the returned scores."""
import ctypes as C

import numpy as np
import pytest

import sim_oracle as so
from _search_set_cases import np_select, round_layout, same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-12           # what tests/test_batch_round_gpu.py holds the batched pass to


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


@pytest.fixture(scope="module")
def cus(gpu):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _features(n, s, e, d, dtype, seed):
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((n, s, e, d), dtype=np.float32))
    x *= np.array([3.8, 1.2, 2.0], dtype=np.float32)[:s].reshape(1, s, 1, 1)
    return x.astype(dtype)                                    # what the database stores (float16: rounded once, here)


def _mask(n, s, e):
    """Missing splits, every (clip, stream) keeping at least one; the pattern depends on the ROW (so a view's position reads another
    clip's bits if the kernel indexes the mask by position)."""
    present = np.ones((n, s, e), dtype=np.uint8)
    present[::7, 0, 0] = 0
    present[3::11, s - 1, e - 1] = 0
    present[n - 1, :, 0] = 0
    present[..., 0] |= (present.sum(axis=2) == 0).astype(np.uint8)
    return present


def _mid(n):
    """a mid-tile row that is neither the clip query 0 is made from nor its duplicate"""
    return (n // 2) // 16 * 16 + 5 if n > 32 else 9


def families(n):
    """name -> strictly ascending rows (None: the whole database).  Those that need more rows than the database has are left out."""
    rows = np.arange(n, dtype=np.int64)
    fam = {"whole": None, "empty": rows[:0], "first": rows[:1], "last": rows[n - 1:], "all_but_one": np.delete(rows, _mid(n)),
           "mod37": rows[3::37], "run": rows[5:5 + min(n - 5, 43)], "edges": rows[(rows % 16 == 0) | (rows % 16 == 15)]}
    fam["mod37_b"] = fam["mod37"].copy()                      # the same rows under a second set id
    for i in range(15):                                       # 100-row views, 1 000 rows apart
        if (i + 1) * 1000 <= n:
            fam["hundred%d" % i] = rows[i * 1000 + 17:i * 1000 + 117]
    if n > 16_384:                                            # the last size of the one-workgroup selection, the first of the three passes
        fam["cap"] = rows[:16_384]
        fam["past_cap"] = rows[:16_385]
    if n > 135_000:
        fam["even"] = rows[::2]
        fam["long_run"] = rows[:135_000]
    return fam


ALL9 = ["all_but_one", "whole", "empty", "first", "last", "mod37", "run", "edges", "mod37_b"]
# (dtype, Q, n, S, E, D, mask, layout, the family of each query -- one set id given to two queries wherever a name repeats)
CASES = [
    (np.float32, 1, 16, 1, 1, 256, False, "rows", ["first"]),                                  # one query, a one-row view
    (np.float32, 16, 33, 2, 5, 1024, False, "rows", ALL9 + ["mod37", "run", "first", "edges", "all_but_one", "empty", "last"]),
    (np.float64, 5, 700, 2, 3, 1024, True, "rows", ["all_but_one", "mod37", "run", "edges", "mod37_b"]),   # unused slots; mask by row
    (np.float16, 16, 1003, 2, 3, 1024, True, "rows", ALL9 + ["hundred0", "run", "run", "edges", "mod37", "empty", "last"]),
    # query 2: a threshold below its minimum, M > 1024 (the fetch path), next to the empty view of query 1
    (np.float32, 9, 4100, 3, 2, 768, True, "rows", ["all_but_one", "empty", "all_but_one", "mod37", "run", "edges", "hundred3", "mod37_b", "last"]),
    # a whole-database query (three-pass selection) beside 100-row views (one-workgroup selection)
    (np.float32, 16, 16_400, 2, 1, 256, False, "rows", ["all_but_one", "whole"] + ["hundred%d" % i for i in range(14)]),
    (np.float32, 9, 4100, 2, 2, 1024, True, "tiled", ["all_but_one", "empty", "all_but_one", "mod37", "run", "edges", "whole", "mod37_b", "last"]),
    # short and long pieces on both sides of kSelSmallN, an empty one and a whole one in one launch set
    (np.float32, 5, 16_400, 1, 1, 256, False, "rows", ["cap", "past_cap", "empty", "whole", "first"]),
    # tiled, no view is whole: untouched tiles, and tiles touched in one clip (mod37, first, last)
    (np.float32, 16, 16_400, 2, 1, 1024, False, "tiled", ["run", "mod37", "first", "last", "mod37_b", "empty"] + ["hundred%d" % i for i in range(10)]),
    # no whole view and a union of more than 512 clips per compute unit: a second round of union tiles
    (np.float32, 16, 140_007, 2, 1, 256, True, "rows", ["long_run", "even"] * 8),
]
# one case per (dtype, D, mask) at n = 203, Q = 5, row-major: with the cases above these launch every VIEW instantiation
SMALL = [(dt, 5, 203, 2, 2, d, m, "rows", ["all_but_one", "mod37", "run", "edges", "empty"])
         for dt in (np.float16, np.float32, np.float64) for d in (256, 512, 768, 1024) for m in (False, True)]
# The instantiations launch_view_pass (csrc/vq_sim_batch.hip) can choose -- batch_view_kernel<T, D / 256, 2, masked, 8, tiled>:
# 24 row-major ones, every (dtype, D, mask), launched by the SMALL cases (and again by CASES), and the two tiled ones (float32, D = 1024,
# plain / masked), launched by the two tiled CASES.  A new storage type, width or layout there gets a new case and a new entry here.
VIEW_KERNELS = {(dt, d, m, "rows") for dt in (np.float16, np.float32, np.float64) for d in (256, 512, 768, 1024) for m in (False, True)}
VIEW_KERNELS |= {(np.float32, 1024, False, "tiled"), (np.float32, 1024, True, "tiled")}
assert VIEW_KERNELS == {(c[0], c[5], c[6], c[7]) for c in CASES + SMALL}


def _case_id(c):
    return "%s-Q%d-n%d-S%dE%dD%d-%s-%s" % (np.dtype(c[0]).name, c[1], c[2], c[3], c[4], c[5], "m" if c[6] else "p", c[7])


@pytest.mark.parametrize("dtype,Q,n,S,E,D,mask,layout,assign", CASES + SMALL, ids=[_case_id(c) for c in CASES + SMALL])
def test_view_round_against_the_batched_round_single_rounds_oracle_and_numpy_partition(vqa, cus, dtype, Q, n, S, E, D, mask, layout, assign):
    """Per query: avg, scores and n_e == query_round_batch's at the view's rows, bit for bit; avg <= 1e-12 from the one-query round
    under use_search_set and from the oracle on x[rows]; lists, counts and near_argmax == the numpy stable partition of the RETURNED
    scores, as view positions; a second call returns the same bits; last_view_round_union == np.unique of the rows."""
    assert len(assign) == Q
    fam = families(n)
    x = _features(n, S, E, D, dtype, seed=n + Q)
    r0, dup = min(7, n - 1), n - 3                             # query 0 is made from clip r0; row dup becomes a copy of it
    assert _mid(n) not in (r0, dup)
    db = vqa.FeatureDB.from_arrays(x, dtype=dtype)
    x[dup] = x[r0]
    db.upload(dup, x[r0:r0 + 1])                              # the duplicate goes in through upload
    present = _mask(n, S, E) if mask else None
    if present is not None:
        present[dup] = present[r0]
    if layout == "tiled":
        db.set_layout("tiled")
    if present is not None:
        db.set_present(present)
    for name in sorted(set(assign)):
        if fam[name] is not None:
            db.define_search_rows(name, fam[name])
    set_ids = [None if fam[name] is None else name for name in assign]
    rows = [np.arange(n, dtype=np.int64) if fam[name] is None else fam[name] for name in assign]
    rng = np.random.default_rng(Q * 1000 + n)
    targets = rng.standard_normal((Q, S, E, D)) / D
    targets[0] = np.stack([[so.scale_feature(x[r0, s, e].astype(np.float64)) for e in range(E)] for s in range(S)])
    weights = 0.5 + rng.random((Q, S))
    ref = db.query_round_batch(targets, weights, None)        # the same queries in the same slots over the whole database
    bands = np.tile([[0.5, 0.1]], (Q, 1))
    for q in range(Q):
        if rows[q].size >= 2:
            lo, hi = np.quantile(ref[q].scores[rows[q]], [0.90, 0.97])
            bands[q] = (hi, lo)
    both = r0 in rows[0] and dup in rows[0]
    if both:
        bands[0] = (2.0, np.quantile(ref[0].scores[rows[0]], 0.5))    # above the maximum: no match; the two copies of r0 are the largest near scores
    if Q > 1:
        bands[1, 1] = bands[1, 0]                             # lower == threshold: no near list
    if Q > 2 and rows[2].size > 1024:
        lowest = ref[2].scores[rows[2]].min()
        bands[2] = (lowest - 1.0, lowest - 2.0)               # everything matches: longer than the prefix

    off, start = (C.c_int64 * 12)(), (C.c_int64 * 17)()
    tokens = (C.c_int32 * Q)(*[-1 if s is None else db._sets[s].token for s in set_ids])
    vqa._lib.call("vq_db_view_round_layout", db._h, Q, tokens, off, start)
    assert (list(off), list(start)) == round_layout(Q, S, E, D, m=[r.size for r in rows])
    got = db.query_round_batch_sets(targets, weights, set_ids, bands)
    assert len(got) == Q
    union = np.unique(np.concatenate(rows))
    if n > 131_072:
        assert not any(s is None for s in set_ids) and union.size > cus * 512       # a second round of union tiles
    assert db.last_view_round_union == (union.size, np.unique(union >> 4).size)
    for q, r in enumerate(got):
        m = rows[q].size
        assert r.scores.shape == (m,) and r.avg.shape == (m, S) and r.n_e.shape == (m, S) and r.n_e.dtype == np.int32, q
        # 1. the bits of the batched round at the view's rows
        assert same_bits(r.avg, ref[q].avg[rows[q]]), q
        assert same_bits(r.scores, ref[q].scores[rows[q]]), q
        assert same_bits(r.n_e, ref[q].n_e[rows[q]]), q
        # 3. the partition, in view positions
        want = np_select(r.scores, bands[q, 0], bands[q, 1])
        assert r.match_rows.dtype == np.int64 and r.near_rows.dtype == np.int64
        assert len(r.match_rows) == len(want[0]) and len(r.near_rows) == len(want[1]), q
        assert (r.match_rows == want[0]).all() and (r.near_rows == want[1]).all() and r.near_argmax == want[2], q
        if m == 0:
            assert r.near_argmax == -1
    if both:
        p0, pd = int(np.searchsorted(rows[0], r0)), int(np.searchsorted(rows[0], dup))
        assert len(got[0].match_rows) == 0 and got[0].near_argmax == min(p0, pd) and got[0].scores[p0] == got[0].scores[pd]
        assert got[0].scores[p0] == got[0].scores[got[0].near_rows].max()
    if Q > 1 and rows[1].size >= 2:
        assert len(got[1].near_rows) == 0 and got[1].near_argmax == -1 and len(got[1].match_rows) > 0
    if Q > 2 and rows[2].size > 1024:
        assert (got[2].match_rows == np.arange(rows[2].size)).all()
    # 4. a second call returns the same bits
    again = db.query_round_batch_sets(targets, weights, set_ids, bands)
    for a, b in zip(got, again):
        assert same_bits(a.scores, b.scores) and same_bits(a.avg, b.avg) and same_bits(a.n_e, b.n_e)
        assert (a.match_rows == b.match_rows).all() and (a.near_rows == b.near_rows).all() and a.near_argmax == b.near_argmax
    # 2. the one-query round under the set, and the oracle on the set's clips
    xo = x.astype(np.float64)
    for q in range(Q):
        if rows[q].size == 0:
            continue
        db.use_search_set(set_ids[q])
        one = db.query_round(targets[q], weights[q], None)
        assert (one.n_e == got[q].n_e).all() and np.abs(one.avg - got[q].avg).max() <= TOL, q
        assert np.abs(one.scores - got[q].scores).max() <= TOL, q
        _, o_avg, o_ne = so.dense_similarities(xo[rows[q]], targets[q], None if present is None else present[rows[q]])
        assert (got[q].n_e == o_ne).all() and np.abs(got[q].avg - o_avg).max() <= TOL, q
        assert np.abs(got[q].scores - so.dense_scores(o_avg, weights[q])).max() <= TOL, q
    db.use_search_set(None)
    db.close()


def _small_db(vqa, n=700, seed=5):
    x = so.cfg1_features(n=n, e=3, seed=seed)
    present = np.ones((n, 2, 3), dtype=np.uint8)
    present[5, 0, 2] = 0
    present[n // 6, 1, :2] = 0
    db = vqa.FeatureDB.from_arrays(x, present=present)
    picks = [(7 + 41 * i) % n for i in range(6)]
    targets = np.stack([np.stack([[so.scale_feature(x[r, s, e].astype(np.float64)) for e in range(3)] for s in range(2)]) for r in picks])
    weights = np.stack([[1.0, 1.5 + 0.1 * i] for i in range(6)])
    return db, x, targets, weights


def test_a_view_round_leaves_the_one_query_state_and_the_set_in_use_alone(vqa):
    """A one-query scan under set A, then a view round over other sets: the one-query scores and similarities read back with the same
    bits, search_set_in_use and vq_db_rows_active are what they were."""
    db, _x, targets, weights = _small_db(vqa)
    db.define_search_rows("A", np.arange(10, 300, 3))
    db.define_search_rows("B", np.arange(250, 600))
    db.use_search_set("A")
    db.set_query(targets[0])
    db.scan(weights[0])
    scores = db.scores().copy()
    avg, ne = (a.copy() for a in db.similarities())
    view, m = C.c_int32(), C.c_int64()
    vqa._lib.call("vq_db_rows_active", db._h, C.byref(view), C.byref(m))
    before = (view.value, m.value)
    got = db.query_round_batch_sets(targets[1:4], weights[1:4], ["B", None, "A"], np.tile([[0.3, 0.1]], (3, 1)))
    assert [r.scores.shape[0] for r in got] == [350, 700, 97]
    assert db.search_set_in_use == "A"
    vqa._lib.call("vq_db_rows_active", db._h, C.byref(view), C.byref(m))
    assert (view.value, m.value) == before == (db._sets["A"].token, 97)
    assert same_bits(db.scores(), scores)
    avg2, ne2 = db.similarities()
    assert same_bits(avg2, avg) and same_bits(ne2, ne)
    db.rescore(weights[3])
    assert (db.scores() == so.dense_scores(avg, weights[3])).all()
    db.use_search_set(None)
    db.close()


def test_after_a_view_round_the_batched_scores_pointer_names_nothing(vqa):
    db, _x, targets, weights = _small_db(vqa, n=300)
    db.define_search_rows("A", np.arange(10, 200, 3))
    lib = vqa.load_library()
    ptr, nq = C.c_void_p(), C.c_int32()
    db.query_round_batch(targets[:3], weights[:3], None)
    assert lib.vq_db_batch_scores_devptr(db._h, C.byref(ptr), C.byref(nq)) == 0 and nq.value == 3
    db.query_round_batch_sets(targets[:2], weights[:2], ["A", "A"], None)
    assert lib.vq_db_batch_scores_devptr(db._h, C.byref(ptr), C.byref(nq)) == -4             # VQ_E_STATE: no [Q][N] array
    db.query_round_batch(targets[:3], weights[:3], None)
    assert lib.vq_db_batch_scores_devptr(db._h, C.byref(ptr), C.byref(nq)) == 0 and nq.value == 3
    db.close()


def test_all_views_empty_launch_nothing_and_report_empty_lists(vqa):
    db, _x, targets, weights = _small_db(vqa, n=100)
    db.define_search_rows("none", np.zeros(0, dtype=np.int64))
    got = db.query_round_batch_sets(targets[:2], weights[:2], ["none", "none"], np.tile([[0.3, 0.1]], (2, 1)))
    for r in got:
        assert r.scores.shape == (0,) and r.avg.shape == (0, 2) and len(r.match_rows) == 0 and len(r.near_rows) == 0 and r.near_argmax == -1
    assert db.last_view_round_union == (0, 0)
    db.close()


def test_refusals(vqa):
    db, _x, targets, weights = _small_db(vqa, n=100)
    lib = vqa.load_library()
    assert lib.vq_db_view_round_union(db._h, None, None) == -4                               # no view round yet
    db.define_search_rows("some", np.arange(10, 60))
    db.define_search_rows("gone", np.arange(5))
    token_gone = db._sets["gone"].token
    db.drop_search_set("gone")
    with pytest.raises(vqa.VqError) as ei:
        db.query_round_batch_sets(targets[:2], weights[:2], ["some", "never"], None)          # a set id that is not defined
    assert ei.value.code == -1 and "query 1" in str(ei.value)
    with pytest.raises(vqa.VqError) as ei:
        db.query_round_batch_sets(targets[:2], weights[:2], ["gone", "some"], None)           # a set that was dropped
    assert ei.value.code == -1 and "query 0" in str(ei.value)
    with pytest.raises(vqa.VqError):
        db.query_round_batch_sets(targets[:0], weights[:0], [], None)                         # Q = 0
    with pytest.raises(vqa.VqError):
        db.query_round_batch_sets(np.zeros((17, 2, 3, 1024)), np.ones((17, 2)), [None] * 17, None)      # Q = 17
    # the library's own checks, at the ctypes level
    views = (C.c_int32 * 2)(db._sets["some"].token, -1)
    off, start = (C.c_int64 * 12)(), (C.c_int64 * 17)()
    vqa._lib.call("vq_db_view_round_layout", db._h, 2, views, off, start)
    assert all(int(v) % 64 == 0 for v in off[:10]) and off[10] == 1024 and off[11] == 150 and list(start[:3]) == [0, 50, 150]
    p = C.c_void_p()
    vqa._lib.call("vq_host_alloc", C.byref(p), int(off[9]))
    assert lib.vq_db_query_round_views(db._h, 2, views, p, int(off[9]) - 1, 7) == -1          # a short block
    assert lib.vq_db_query_round_views(db._h, 2, views, p, int(off[9]), 16) == -1             # an unknown flag
    assert lib.vq_db_query_round_views(db._h, 2, None, p, int(off[9]), 7) == -1               # NULL views
    bad = (C.c_int32 * 2)(db._sets["some"].token, token_gone)
    assert lib.vq_db_query_round_views(db._h, 2, bad, p, int(off[9]), 7) == -1
    assert b"query 1" in lib.vq_last_error()
    bad = (C.c_int32 * 2)(-2, -1)
    assert lib.vq_db_view_round_layout(db._h, 2, bad, off, start) == -1 and b"query 0" in lib.vq_last_error()
    assert lib.vq_db_query_round_views(db._h, 2, views, p, int(off[9]), 7) == 0
    vqa._lib.call("vq_host_free", p)
    db.close()
