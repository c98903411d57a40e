"""GPU, one handle: the two calls of include/vq_amd_round_shard.h.  FeatureDB.batch_round_avg_rows against avg[rows] of the round's own
results, as bits; FeatureDB.batch_round_update_given, fed those tables, against FeatureDB.batch_round_update on the same round with ==
on every field -- pick, lowest, band, flags, scores, partitions and the surface -- at the label counts either side of the fit's chunk
(4096 | 4097), the user-row counts either side of the fold's one-row-per-thread (256 | 257) and well above it, on a whole-database
round and on a view round over three search sets; a presence-masked database where a labelled row's average is NaN; the refusals."""
import ctypes as C

import numpy as np
import pytest

import _pick_cases as pc
import test_batch_tickets_gpu as base
import test_batch_update_gpu as upd

pytestmark = pytest.mark.gpu
N, E, Q, BALLAST, NEAR = 300, 2, 5, 0.3, 0.35
SETS = {"a": sorted(set(range(3, N, 7)) | {upd.FAR, upd.NANROW} | set(upd.refs())), "b": list(range(2, N - 20)), "c": list(range(0, N, 2))}
ROUNDS = {"whole": [None] * Q, "views": ["a", None, "b", "c", "a"]}
# (query, L, U; U None: a revise member): not in query order, a skipped slot, both band modes; every L of 1 | 13 | 4096 | 4097 and every U of
# 0 | 1 | 256 | 257 | 600 occurs
GROUPS = {"chunk-edge": [(3, 4097, 257), (0, 1, None), (4, 13, 600), (1, 0, 3), (2, 4096, 0)],
          "fold-edge": [(1, 13, 1), (0, 4096, 256), (2, 7, None)]}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    if base.X is None:
        base.X = base.features()
    return m


def make_db(vqa, present=None):
    x, t = upd.data(N, E)
    db = vqa.FeatureDB.from_arrays(x, present=present)
    for sid, rows in SETS.items():
        db.define_search_rows(sid, np.array(rows, dtype=np.int64))
    return db, t


def run_round(db, t, sets):
    w0 = np.array([[1.0, 0.6 + 0.1 * q] for q in range(Q)])
    bands0 = np.array([[0.8, 0.73]] * Q)
    results = db.query_round_batch_sets(t[:Q], w0, sets, bands0) if any(s is not None for s in sets) else db.query_round_batch(t[:Q], w0, bands0)
    return [(np.array(r.avg), np.array(r.scores)) for r in results]


@pytest.fixture(scope="module")
def rounds(vqa):
    """kind -> (database, [(avg, scores) per query]): one round of each kind, shared; the updates behind it rewrite scores and lists of
    their slots only, and both calls read nothing but the round's avg."""
    out = {}
    for kind, sets in ROUNDS.items():
        db, t = make_db(vqa)
        out[kind] = (db, run_round(db, t, sets))
    yield out
    for db, _r in out.values():
        db.close()


def grids(vqa):
    hp = pc.make_hp(vqa)
    return pc.candidates(hp), np.asarray(hp.threshold_grid, dtype=np.float64), pc.compute_eps()


def members_of(group, kept, seed):
    """(queries, rows, labels, reaches, users): rows drawn WITH repetition from the query's piece, the better half confirmed and one
    verdict in ten flipped; the user rows ascending, as a ticket hands them over."""
    rng = np.random.default_rng(seed)
    queries, rows, labels, reaches, users = [], [], [], [], []
    for q, L, U in group:
        scores = kept[q][1]
        m = scores.shape[0]
        r = rng.integers(0, m, size=L).astype(np.int64)
        r[np.isnan(scores[r])] = 0                                            # the row of NaN features carries no label here (it would make
        y = ((scores[r] >= (np.median(scores[r]) if L else 0.0)) ^ (rng.random(L) < 0.1)).astype(np.float64)      # the whole surface NaN)
        queries.append(q)
        rows.append(r)
        labels.append(y)
        reaches.append(NEAR if U is None else None)
        users.append(np.sort(rng.integers(0, m, size=U or 0)).astype(np.int64))
    return queries, rows, labels, reaches, users


def tables(db, queries, rows, users):
    """The labelled and the user rows' averaged similarities through ONE batch_round_avg_rows call, an entry's two lists in one."""
    both = [np.concatenate([r, u]) for r, u in zip(rows, users)]
    have = [i for i, b in enumerate(both) if b.size]
    got = dict(zip(have, db.batch_round_avg_rows([queries[i] for i in have], [both[i] for i in have])))
    S = db.S
    label_avgs = [np.array(got[i][:rows[i].size]) if i in got else np.zeros((0, S)) for i in range(len(queries))]
    user_avgs = [np.array(got[i][rows[i].size:]) if i in got else np.zeros((0, S)) for i in range(len(queries))]
    return label_avgs, user_avgs


def snapshot(r):
    copy = lambda v: None if v is None else np.array(v)                       # noqa: E731
    return (r.w, r.threshold, r.lowest, r.band, r.iw, r.it, r.on_rim, r.fell_back, r.near_argmax), copy(r.scores), copy(r.match_rows), \
        copy(r.near_rows), copy(r.surface)


def same_update(a, b, what):
    (pick_a, sc_a, m_a, k_a, sf_a), (pick_b, sc_b, m_b, k_b, sf_b) = a, b
    if pick_b[0] is None:                                                     # a skipped slot
        assert pick_a == pick_b and sc_a is None and m_a is None and k_a is None and sf_a is None, what
        return
    assert pick_a[4:] == pick_b[4:] and same_bits(pick_a[:3], pick_b[:3]) and same_bits(pick_a[3], pick_b[3]), (what, pick_a, pick_b)
    assert (sc_a is None) == (sc_b is None) and (sc_b is None or same_bits(sc_a, sc_b)), what
    assert np.array_equal(m_a, m_b) and np.array_equal(k_a, k_b), what
    assert (sf_a is None) == (sf_b is None) and (sf_b is None or same_bits(sf_a, sf_b)), what


@pytest.mark.parametrize("kind", sorted(ROUNDS))
def test_avg_rows_are_the_rounds_own_bits(vqa, rounds, kind):
    db, kept = rounds[kind]
    rng = np.random.default_rng(3)
    queries = [4, 0, 2, 3]                                                    # not in query order; query 1 is left out
    nan_at = [i for i, r in enumerate(SETS["a"]) if r == upd.NANROW][0] if kind == "views" else upd.NANROW
    rows = [np.concatenate([[nan_at, 0, kept[q][0].shape[0] - 1, 0], rng.integers(0, kept[q][0].shape[0], size=n)]) for q, n in zip(queries, (5, 1, 700, 33))]
    rows[1] = np.zeros(0, dtype=np.int64)                                     # an entry without rows
    got = db.batch_round_avg_rows(queries, rows)
    assert got[1] is None
    for q, r, a in zip(queries, rows, got):
        if r.size:
            assert a.shape == (r.size, db.S) and a.dtype == np.float64 and same_bits(a, kept[q][0][r]), q
    assert np.isnan(got[0][0]).all()                                          # the row of NaN features came through as it was


@pytest.mark.parametrize("kind,group", [(k, g) for k in sorted(ROUNDS) for g in sorted(GROUPS)])
def test_update_given_equals_update(vqa, rounds, kind, group):
    db, kept = rounds[kind]
    cand, ths, eps = grids(vqa)
    queries, rows, labels, reaches, users = members_of(GROUPS[group], kept, len(kind) + len(group))
    k = len(queries)
    common = ([cand] * k, [ths] * k, [BALLAST] * k, [1] * k, eps, reaches)
    want = [snapshot(r) for r in db.batch_round_update(queries, rows, labels, *common, users, want_surface=True)]
    label_avgs, user_avgs = tables(db, queries, rows, users)
    for q, r, u, la, ua in zip(queries, rows, users, label_avgs, user_avgs):
        assert same_bits(la, kept[q][0][r]) and same_bits(ua, kept[q][0][u]), q
    got = [snapshot(r) for r in db.batch_round_update_given(queries, labels, label_avgs, *common, user_avgs, want_surface=True)]
    for q, a, b in zip(queries, got, want):
        print(kind, group, "query", q, "pick", b[0])
        same_update(a, b, (kind, group, q))
    served = [b for b in want if b[0][0] is not None]
    assert len(served) == sum(1 for _q, L, _U in GROUPS[group] if L) and any(len(b[2]) + len(b[3]) for b in served)
    for b, (_q, L, U) in zip(want, GROUPS[group]):                            # lowest: 1.0 without user rows, below it with hundreds of them
        assert L == 0 or (b[0][2] == 1.0 if not U else b[0][2] < 1.0 or U < 256), (L, U, b[0])
    assert any(not b[0][6] for b in served), "every pick lies on the rim of the grid: the refinement is not exercised"
    lean = [snapshot(r) for r in db.batch_round_update_given(queries, labels, label_avgs, *common, user_avgs, want_scores=False)]
    for q, a, b in zip(queries, lean, want):
        same_update((a[0], b[1] if a[0][0] is not None else None, a[2], a[3], b[4] if a[0][0] is not None else None), b, (kind, group, q, "lean"))
        assert a[1] is None and a[4] is None


def test_a_nan_average_travels_as_bits(vqa):
    """A presence mask without any split of stream 1 for row 21: its average is 0 / 0.  Labelled and confirmed, the row goes through the
    tables and both calls still agree bit for bit (the whole surface of that member is NaN: the pick is cell (0, 0))."""
    x, _t = upd.data(N, E)
    present = np.ones((N, 2, E), dtype=np.uint8)
    present[21, 1, :] = 0
    db, t = make_db(vqa, present=present)
    kept = run_round(db, t, ROUNDS["whole"])
    assert np.isnan(kept[0][0][21, 1]) and not np.isnan(kept[0][0][21, 0])
    cand, ths, eps = grids(vqa)
    queries = [2, 0]
    rows = [np.array([30, 21, 7, 30, 100]), np.array([14, 15, 16, 40, 41, 200, 250])]
    labels = [np.array([1.0, 1.0, 0.0, 1.0, 0.0]), np.array([1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0])]
    users = [np.array([21, 30]), np.array([14, 21])]
    common = ([cand] * 2, [ths] * 2, [BALLAST] * 2, [1] * 2, eps, [None, None])
    want = [snapshot(r) for r in db.batch_round_update(queries, rows, labels, *common, users, want_surface=True)]
    label_avgs, user_avgs = tables(db, queries, rows, users)
    assert np.isnan(label_avgs[0][1, 1]) and np.isnan(user_avgs[1][1, 1])
    for q, r, u, la, ua in zip(queries, rows, users, label_avgs, user_avgs):
        assert same_bits(la, kept[q][0][r]) and same_bits(ua, kept[q][0][u])
    got = [snapshot(r) for r in db.batch_round_update_given(queries, labels, label_avgs, *common, user_avgs, want_surface=True)]
    for q, a, b in zip(queries, got, want):
        same_update(a, b, q)
    assert np.isnan(want[0][4]).all() and want[0][0][4:6] == (0, 0) and not np.isnan(want[1][4]).any()
    assert np.isfinite(want[1][0][2]) and want[1][0][2] < 1.0                 # the NaN score of the confirmed row 21 is skipped by the fold
    db.close()


def test_layouts_on_a_real_handle_size_the_row_pieces_by_its_streams(vqa, rounds):
    db, _kept = rounds["whole"]
    lib = vqa.load_library()
    S = db.S
    assert S == 2
    off, plain, rows = (C.c_int64 * 16)(), (C.c_int64 * 16)(), (C.c_int64 * 4)()
    for q, g, t, nl, nu in ((16, 64, 64, 4097, 333), (1, 1, 1, 0, 0), (3, 40, 31, 7, 0)):
        assert lib.vq_db_batch_update_given_layout(db._h, q, g, t, nl, nu, off) == 0 and lib.vq_db_batch_update_layout(db._h, q, g, t, nl, nu, plain) == 0
        o, p = list(off), list(plain)
        assert all(v % 64 == 0 for v in o) and o == sorted(o)
        assert o[5] - o[4] == (nl * S * 8 + 63) // 64 * 64 and o[13] - o[12] == (nu * S * 8 + 63) // 64 * 64
        assert all(o[i + 1] - o[i] == p[i + 1] - p[i] for i in range(15) if i not in (4, 12))
        assert lib.vq_db_batch_avg_rows_layout(db._h, q, nl, rows) == 0
        assert rows[3] - rows[2] == (nl * S * 8 + 63) // 64 * 64 and rows[2] - rows[1] >= nl * 8 and rows[1] >= q * 8


def test_refusals_are_argument_checks_and_leave_the_round_usable(vqa, monkeypatch):
    import sys
    db, t = make_db(vqa)
    cand, ths, eps = grids(vqa)
    rows, y = np.array([20, 31, 299], dtype=np.int64), np.array([1.0, 0.0, 1.0])
    avg3, user1 = np.full((3, 2), 0.5), np.full((1, 2), 0.25)

    def given(q=1, y=y, label_avg=avg3, second=1, reach=None, user_avg=user1, **kw):
        return db.batch_round_update_given([q], [y], [label_avg], [cand], [ths], [BALLAST], [second], eps, [reach], [user_avg], **kw)

    def refused(code, call, *a, **kw):
        with pytest.raises(vqa.VqError) as ei:
            call(*a, **kw)
        assert ei.value.code == code, str(ei.value)
    refused(-4, given)                                                        # no batched round yet
    refused(-4, db.batch_round_avg_rows, [1], [rows])
    kept = run_round(db, t, ROUNDS["whole"])
    refused(-4, given, q=5)                                                   # a slot the round lacked (5 queries)
    refused(-4, db.batch_round_avg_rows, [5], [rows])
    refused(-1, db.batch_round_avg_rows, [1], [np.array([20, N])])            # a row = M_q
    refused(-1, db.batch_round_avg_rows, [1], [np.array([-1, 20])])
    refused(-1, given, second=2)                                              # S = 2
    fdb = sys.modules[vqa.FeatureDB.batch_round_update.__module__]
    real = fdb.call

    def one_more(name, *a):                                                   # sum L != n_labels | n_rows: the counts of the call and of the block differ
        if name == "vq_db_batch_round_update_given":
            a = a[:4] + (a[4] + 1,) + a[5:]
        if name == "vq_db_batch_round_avg_rows":
            a = a[:2] + (a[2] + 1,) + a[3:]
        return real(name, *a)
    monkeypatch.setattr(fdb, "call", one_more)
    refused(-1, given)
    refused(-1, db.batch_round_avg_rows, [1], [rows])

    def given_surface(name, *a):                                              # the flag of the one-handle call is not this call's
        if name == "vq_db_batch_round_update_given":
            a = a[:-1] + (a[-1] | vqa._lib.VQ_BUPDATE_GIVEN_SURFACE,)
        return real(name, *a)
    monkeypatch.setattr(fdb, "call", given_surface)
    refused(-1, given)
    monkeypatch.setattr(fdb, "call", real)
    # nothing was launched: the device still holds the round's scores, and both calls then work
    dev = upd.device_scores(vqa, db, Q, N)
    assert all(same_bits(dev[q], kept[q][1]) for q in range(Q))
    la, ua = tables(db, [1], [rows], [np.array([7])])
    want = snapshot(db.batch_round_update([1], [rows], [y], [cand], [ths], [BALLAST], [1], eps, [None], [np.array([7])], want_surface=True)[0])
    same_update(snapshot(given(label_avg=la[0], user_avg=ua[0], want_surface=True)[0]), want, "after the refusals")
    db.close()
