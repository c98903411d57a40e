"""GPU: the scores of chosen rows of a batched round under a grid of weights (include/vq_amd_round_grid.h, FeatureDB.batch_round_grid)
against the one-query scores_grid on a second, identical database that got the round's averaged similarities through write_avg, and
against the round's own scores.  Everything is compared with ==.

The shapes, and what each can expose:
  N = 37, S = 2, E = 3, D = 256, fp32   two full 16-row tiles and a ragged five: a piece offset (qoff) that is no multiple of a tile,
                                        so a wrong query stride reads another query's avg
  rows 0 and 36, a repeated row         the first and the last entry of a piece (an off-by-one in the row bound), and two threads
                                        that read one entry
  a query without rows                  a slot whose workgroups must all leave; the pieces of `graded` behind it must not shift
  G in {1, 40}                          the g / l split of a thread's index at its degenerate and at the reference's size
  300 rows with G = 3                   (g, l) crosses 256-thread workgroups: 900 threads, the last workgroup ragged
  N = 16, S = 8, E = 1                  the [8] stride of w_grid equals S: a kernel that strode by S would pass every other case"""
import numpy as np
import pytest

import sim_oracle as so

pytestmark = pytest.mark.gpu
VQ_E_INVALID, VQ_E_STATE = -1, -4
N = 37
W = np.array([[1.0, 1.5], [1.0, 0.8], [1.0, 2.0]])
BANDS = np.array([[0.8, 0.6]] * 3)
REFS = (3, 20, 36)
ROWS = [np.array([0, 36, 5, 5, 17]), np.zeros(0, dtype=np.int64), np.array([36, 0, 16, 15, 31, 32, 0])]


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def targets(x, refs):
    _n, s, e, _d = x.shape
    return np.stack([np.stack([[so.scale_feature(x[r, si, ei].astype(np.float64)) for ei in range(e)] for si in range(s)]) for r in refs])


@pytest.fixture(scope="module")
def case(vqa):
    """(db, ref, x, t, results): the round of three queries on the 37-clip database, run once and left unchanged."""
    x = so.synth_features(7, 0, N, 2, 3, 256, (4.0, 1.0))
    db, ref = vqa.FeatureDB.from_arrays(x), vqa.FeatureDB.from_arrays(x)
    t = targets(x, REFS)
    return db, ref, x, t, db.query_round_batch(t, W, BANDS)


def grid40(vqa, S):
    hp = vqa.Hyperparameter({"rgb": 1.0, "warped_optical_flow": 1.5})
    cand = np.zeros((len(hp.weight_grid), S))
    cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
    assert cand.shape[0] == 40
    return cand


def one_query_grid(ref, r, w_grid, rows):
    ref.write_avg(np.array(r.avg), np.array(r.n_e))
    return ref.scores_grid(w_grid, rows)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


@pytest.mark.parametrize("G", [1, 40])
def test_grid_scores_equal_scores_grid_on_the_same_avg(vqa, case, G):
    db, ref, _x, _t, results = case
    cand = grid40(vqa, 2)[:G] if G > 1 else np.array([[1.0, 1.3]])
    grids = [cand, cand * 0.5 + 0.25, cand[::-1].copy()]              # another grid per query: a wrong q in the w_grid index shows
    got = db.batch_round_grid([0, 1, 2], ROWS, grids)
    assert got[1] is None
    for q in (0, 2):
        assert got[q].shape == (G, len(ROWS[q])) and np.isfinite(got[q]).all()
        assert same(got[q], one_query_grid(ref, results[q], grids[q], ROWS[q])), q
    # entries in another order than the round's queries, and a single query that is not the first
    back = db.batch_round_grid([2, 0], [ROWS[2], ROWS[0]], [grids[2], grids[0]])
    assert same(back[0], got[2]) and same(back[1], got[0])
    assert same(db.batch_round_grid([1], [ROWS[0]], [grids[1]])[0], one_query_grid(ref, results[1], grids[1], ROWS[0]))


def test_with_the_rounds_weights_the_grid_score_is_the_rounds_score(vqa, case):
    db, _ref, _x, _t, results = case
    rows = [np.arange(N), np.array([36, 0]), ROWS[2]]
    got = db.batch_round_grid([0, 1, 2], rows, [W[q][None, :] for q in range(3)])
    for q in range(3):
        assert same(got[q][0], np.asarray(results[q].scores)[rows[q]]), q
    # the snapshot and the one-query state were not written: the round's lists are still served, a rescore still works on its avg
    again = db.batch_round_topk(5)
    for q in range(3):
        order = np.lexsort((np.arange(N), -np.asarray(results[q].scores)))[:5]
        assert same(again[q][0], order.astype(np.int64)) and same(again[q][1], np.asarray(results[q].scores)[order])


def test_three_hundred_rows_cross_the_workgroups(vqa, case):
    db, ref, _x, _t, results = case
    rows = np.random.default_rng(3).integers(0, N, size=300).astype(np.int64)
    rows[[0, 255, 256, 299]] = (36, 0, 36, 0)
    cand = grid40(vqa, 2)[[0, 17, 39]]
    got = db.batch_round_grid([1, 2], [rows, rows[:7]], [cand, cand])
    assert got[0].shape == (3, 300)
    assert same(got[0], one_query_grid(ref, results[1], cand, rows)) and same(got[1], one_query_grid(ref, results[2], cand, rows[:7]))


def test_after_a_rescore_the_grid_score_is_the_rescored_score(vqa):
    x = so.synth_features(7, 0, N, 2, 3, 256, (4.0, 1.0))
    db = vqa.FeatureDB.from_arrays(x)
    t = targets(x, REFS)
    db.query_round_batch(t, W, BANDS, want_avg=False, want_scores=False)          # nothing copied back: the snapshot alone serves
    new_w = np.array([[1.0, 0.55], [1.0, 2.4]])
    rescored = db.batch_round_rescore([2, 0], new_w, np.array([[0.7, 0.5]] * 2))
    rows = np.array([0, 36, 11, 11, 16])
    got = db.batch_round_grid([0, 2], [rows, np.arange(N)], [new_w[1][None, :], new_w[0][None, :]])
    assert same(got[0][0], np.asarray(rescored[1].scores)[rows]) and same(got[1][0], np.asarray(rescored[0].scores))
    # the value of a partition's near arg-max, as a sharded round without scores fetches it
    for r, q, w in ((rescored[0], 2, new_w[0]), (rescored[1], 0, new_w[1])):
        if r.near_argmax >= 0:
            assert db.batch_round_grid([q], [[r.near_argmax]], [w[None, :]])[0][0, 0] == r.scores[r.near_argmax]


def test_rows_of_a_view_round_are_positions_in_the_set(vqa):
    x = so.synth_features(7, 0, N, 2, 3, 256, (4.0, 1.0))
    db = vqa.FeatureDB.from_arrays(x)
    members = np.array([1, 2, 5, 8, 13, 16, 21, 30, 33, 35, 36])                    # 11 rows, the last clip among them
    db.define_search_rows("eleven", members)
    t = targets(x, REFS[:2])
    results = db.query_round_batch_sets(t, W[:2], ["eleven", None], BANDS[:2])
    pos = [np.array([0, 10, 4, 4]), np.array([36, 0, 11])]
    got = db.batch_round_grid([0, 1], pos, [W[0][None, :], W[1][None, :]])
    assert results[0].scores.shape == (11,)
    assert same(got[0][0], np.asarray(results[0].scores)[pos[0]]) and same(got[1][0], np.asarray(results[1].scores)[pos[1]])
    with pytest.raises(vqa.VqError) as ei:                                            # a row equal to M_q of the VIEW (11), valid in the database
        db.batch_round_grid([0], [[11]], [W[0][None, :]])
    assert ei.value.code == VQ_E_INVALID
    kept = np.array(got[0][0])
    whole = db.query_round_batch(t, W[:2])
    assert same(kept, np.asarray(whole[0].scores)[members[pos[0]]])                 # position 10 of the set is row 36 of the database


def test_eight_streams_w_grid_stride_equals_s(vqa):
    x = so.synth_features(9, 0, 16, 8, 1, 256, tuple(np.linspace(4.0, 1.0, 8)))
    db, ref = vqa.FeatureDB.from_arrays(x), vqa.FeatureDB.from_arrays(x)
    t = targets(x, (0, 15))
    w = np.array([np.linspace(1.0, 2.4, 8), np.linspace(2.0, 0.6, 8)])
    results = db.query_round_batch(t, w)
    grid = np.random.default_rng(1).uniform(0.5, 2.5, size=(5, 8))
    rows = [np.array([15, 0, 7, 7]), np.arange(16)]
    got = db.batch_round_grid([0, 1], rows, [grid, grid[::-1].copy()])
    assert same(got[0], one_query_grid(ref, results[0], grid, rows[0])) and same(got[1], one_query_grid(ref, results[1], grid[::-1].copy(), rows[1]))
    own = db.batch_round_grid([0, 1], rows, [w[0][None, :], w[1][None, :]])
    assert same(own[0][0], np.asarray(results[0].scores)[rows[0]]) and same(own[1][0], np.asarray(results[1].scores))


def test_errors_leave_the_snapshot_usable(vqa):
    x = so.synth_features(7, 0, N, 2, 3, 256, (4.0, 1.0))
    db = vqa.FeatureDB.from_arrays(x)
    one = np.array([[1.0, 1.5]])

    def refused(code, queries, rows, grids):
        with pytest.raises(vqa.VqError) as ei:
            db.batch_round_grid(queries, rows, grids)
        assert ei.value.code == code, (ei.value, queries)

    refused(VQ_E_STATE, [0], [[0]], [one])                                            # no batched round on the handle
    results = db.query_round_batch(targets(x, REFS), W, BANDS)

    def valid():
        got = db.batch_round_grid([2], [[36, 0]], [W[2][None, :]])
        assert same(got[0][0], np.asarray(results[2].scores)[[36, 0]])
    valid()
    for code, queries, rows, grids in ((VQ_E_INVALID, [0], [[N]], [one]),             # a row equal to M_q
                                       (VQ_E_INVALID, [1], [[0, -1]], [one]),
                                       (VQ_E_STATE, [3], [[0]], [one]),               # a slot the round did not have
                                       (VQ_E_INVALID, [16], [[0]], [one]),            # Q = 17
                                       (VQ_E_INVALID, [0], [[0]], [np.ones((65, 2))])):      # G = 65
        refused(code, queries, rows, grids)
        valid()
