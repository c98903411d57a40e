"""GPU: FeatureDB.batch_targets (vq_db_batch_targets, csrc/vq_round_targets.hip) -- every draw of every query of a group in one call.

The contract is equality of bits, so there is no tolerance here: the reference of every comparison is the per-ticket path on the same
handle, ``FeatureDB.bootstrap_target(..., set_query=False)`` per draw, with the host side in the parent's expressions (numpy's
``np.average`` over the draws, the blend of ``TargetClip``'s partial_update), and every assertion is ``array_equal``.  The data is
tests/_bootstrap_cases.py's resident block (or a block made the same way for other row counts): every value is exact in its storage
type.  Refusals are status returns of kernels that complete (no device fault involved)."""
import ctypes as C
import random

import numpy as np
import pytest

import _bootstrap_cases as bc
from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS, golden_json, golden_npy, records_from_dense

pytestmark = pytest.mark.gpu
NP = {"float16": np.float16, "float32": np.float32, "float64": np.float64}


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def _block(N, S, E, D, dtype, seed=0):
    """[N][S][E][D] the way _bootstrap_cases.resident_block makes its 12 rows (that block itself for N = 12)."""
    if N == bc.RES_N and seed == 0:
        return bc.resident_block(S, E, D, dtype)
    rng = np.random.default_rng(7000 + 100 * S + 10 * E + D + 13 * N + seed)
    x = np.abs(rng.standard_normal((N, S, E, D))) * 10.0 ** rng.uniform(-bc.RES_SPREAD, bc.RES_SPREAD, (N, S, E, 1))
    x = x.astype(NP[dtype])
    assert np.isfinite(x).all()
    return x


def _reference(db, pool, draws, mu, previous=None, keep=None):
    """The parent's path: one bootstrap_target per draw, np.average over the draws, the blend of partial_update."""
    valid, invalid = pool
    bags = [db.bootstrap_target([valid[i] for i in pv], [invalid[i] for i in pi], mu=mu, set_query=False) for pv, pi in draws]
    t = bags[0] if len(bags) == 1 else np.average(bags, axis=0)
    if previous is not None:
        t = np.multiply(keep, t) + np.multiply((1 - keep), previous)
    return t


def _check(db, pools, draws, mus, previous=None, keeps=None, what=""):
    got = db.batch_targets(pools, draws, mus, previous=previous, keeps=keeps)
    assert len(got) == len(pools)
    for q, t in enumerate(got):
        want = _reference(db, pools[q], draws[q], mus[q], None if previous is None else previous[q], None if keeps is None else keeps[q])
        assert t.shape == want.shape == (db.S, db.E, db.D) and np.isfinite(want).all()
        assert np.array_equal(t, want), "%s query %d: %d of %d values differ, max |d| %.3e" % (
            what, q, int((t != want).sum()), t.size, float(np.abs(t - want).max()))
    return [np.array(t) for t in got]


V, I = list(bc.RES_VALID), list(bc.RES_INVALID)
# pool, draws, mu: every draw shape of the issue on the 12-row block
DRAW_SHAPES = [
    (([5], []), [([0], [])], 0.3),                                                       # a pool of one match and nothing else
    ((V, I), [([0, 1, 2, 3], [0, 1, 2]), ([2, 0, 3], [1, 0]), ([1], [2])], 0.3),          # the whole pool | not ascending | another size
    ((V, []), [([0, 1, 2, 3], []), ([3, 1], [])], 0.3),                                  # no non-matches, two draws of different sizes
    ((V, I), [([0, 1, 3], [0, 2])], 0.0),                                                # mu = 0 with non-matches present
]


@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
@pytest.mark.parametrize("D", [4, 68, 260, 1024])
def test_draw_shapes_on_every_width_and_storage_type(vqa, D, dtype):
    """D below the 64-lane stride, past it, past the 256 threads of the combination, and the product's."""
    db = vqa.FeatureDB.from_arrays(_block(12, 2, 3, D, dtype))
    try:
        _check(db, [s[0] for s in DRAW_SHAPES], [s[1] for s in DRAW_SHAPES], [s[2] for s in DRAW_SHAPES], what="D%d %s" % (D, dtype))
    finally:
        db.close()


def test_tiled_layout_gives_the_bits_of_the_rows_layout(vqa):
    """N = 40: two whole tiles of 16 clips and a ragged one; rows at the edges of all three."""
    x = _block(40, 2, 3, 1024, "float32")
    pools = [([0, 15, 16, 31, 39], [32, 1, 17]), ([38, 2], [])]
    draws = [[([0, 1, 2, 3, 4], [0, 1, 2]), ([4, 2, 0], [1])], [([0, 1], [])]]
    out = []
    for layout in ("rows", "tiled"):
        db = vqa.FeatureDB.from_arrays(x)
        try:
            db.set_layout(layout)
            assert db.layout == layout
            out.append(_check(db, pools, draws, [0.3, 0.0], what=layout))
        finally:
            db.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _ragged_group(rng, Q, N, max_pool=19, many_draws_at=None):
    pools, draws, mus = [], [], []
    for q in range(Q):
        r = 1 + (q * 7) % max_pool if Q > 1 else 9                                          # 1 .. 19 rows, ragged
        rows = rng.permutation(N)[:r].tolist()
        m = max(1, r - r // 3)
        valid, invalid = rows[:m], rows[m:]
        B = 64 if q == many_draws_at else 1 + q % 4
        ds = []
        for _ in range(B):
            pv = rng.permutation(m)[:int(rng.integers(1, m + 1))].tolist()
            pi = rng.permutation(r - m)[:int(rng.integers(0, r - m + 1))].tolist() if r > m else []
            ds.append((pv, pi))
        pools.append((valid, invalid))
        draws.append(ds)
        mus.append([0.3, 0.0, 1.5, 40.0][q % 4])
    return pools, draws, mus


def test_groups_of_one_and_sixteen_reuse_and_grow_the_buffers(vqa):
    """Q = 1, the same call again (same bits: the handle's buffers are reused), then Q = 16 with ragged pools (1 .. 19 rows), ragged
    draw counts (1, 3 and 64 among them) and a mu per query (the buffers grow), and that call again."""
    db = vqa.FeatureDB.from_arrays(_block(40, 2, 3, 68, "float32"))
    try:
        rng = np.random.default_rng(16)
        one = _ragged_group(rng, 1, 40)
        first = _check(db, *one, what="Q1")
        again = db.batch_targets(*one)
        assert np.array_equal(first[0], again[0])
        big = _ragged_group(rng, 16, 40, many_draws_at=5)
        assert sorted({len(d) for d in big[1]}) == [1, 2, 3, 4, 64] and {len(v) + len(i) for v, i in big[0]} >= {1, 19}
        first = _check(db, *big, what="Q16")
        again = db.batch_targets(*big)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        _check(db, *one, what="Q1 after Q16")
    finally:
        db.close()


def test_draws_on_either_side_of_the_local_memory_threshold(vqa):
    """A draw of exactly the largest size solved in local memory and one a row longer (the scratch area), in ONE query, with and
    without non-matches; the threshold is the library's (read through the layout call)."""
    probe = vqa.FeatureDB.from_arrays(_block(12, 1, 1, 4, "float32"))
    T = probe.batch_targets_lds_rows()
    probe.close()
    assert 8 <= T < 255
    N = T + 3
    db = vqa.FeatureDB.from_arrays(_block(N, 1, 2, 260, "float32"))
    try:
        m = T // 2
        valid, invalid = list(range(m)), list(range(m, T + 1))                               # T + 1 rows in the pool
        n = len(invalid)
        at = [(list(range(m)), list(range(n - 1))), (list(range(m)), list(range(n)))]        # T rows | T + 1 rows
        _check(db, [(valid, invalid)], [at], [0.3], what="threshold, with non-matches")
        only = list(range(T + 1))
        _check(db, [(only, [])], [[(only[:T], []), (only, [])]], [0.3], what="threshold, matches only")
    finally:
        db.close()


def test_a_pool_and_a_draw_of_256_rows(vqa):
    """Case(128, 128, 1024, 1, 0.3)-sized: the largest pool, solved in the scratch area, beside a small draw of the same pool."""
    db = vqa.FeatureDB.from_arrays(_block(260, 1, 1, 1024, "float32"))
    try:
        rows = np.random.default_rng(256).permutation(260)[:256].tolist()
        pool = (rows[:128], rows[128:])
        whole = (list(range(128)), list(range(128)))
        _check(db, [pool], [[whole, ([5, 3, 100], [7, 120])]], [0.3], what="R256")
    finally:
        db.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_blend_of_partial_update(vqa, dtype):
    db = vqa.FeatureDB.from_arrays(_block(12, 2, 3, 260, dtype))
    try:
        rng = np.random.default_rng(75)
        prev = [rng.standard_normal((2, 3, 260)) * 1e-2, None, rng.standard_normal((2, 3, 260))]
        pools = [(V, I), (V, I), (V, [])]
        draws = [[([0, 2, 3], [1])], [([0, 1], [0, 2]), ([3], [1])], [([1, 2], [])]]
        got = _check(db, pools, draws, [0.3, 0.3, 0.0], previous=prev, keeps=[0.5, None, 0.7], what="blend " + dtype)
        plain = db.batch_targets(pools, draws, [0.3, 0.3, 0.0])
        assert not np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and not np.array_equal(got[2], plain[2])
    finally:
        db.close()


@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
def test_a_singular_query_among_good_ones(vqa, dtype):
    """The pool of query 1 lists a row twice (the inputs tests/test_bootstrap_edges_gpu.py refuses through the one-draw call): its
    status is 1, it is the query named, the other queries are solved to their references' bits and the handle goes on working."""
    db = vqa.FeatureDB.from_arrays(_block(12, 1, 1, 260, dtype))
    try:
        twice, mu = bc.RES_TWICE[dtype]
        inv = I if mu else []
        with pytest.raises(vqa.VqError) as alone:
            db.bootstrap_target(twice, inv, mu=mu, set_query=False)
        assert alone.value.code == -1 and "singular system" in str(alone.value)
        pools = [(V, I), (twice, inv), (V, [])]
        draws = [[([0, 1, 2, 3], [0, 1, 2])], [([2], []), (list(range(len(twice))), list(range(len(inv))))], [([0, 3], [])]]   # query 1: a good draw, then the whole pool
        mus = [0.3, mu, 0.0]
        status, targets = db._batch_targets_raw(pools, draws, mus)
        assert status[:, 0].tolist() == [0, 1, 0] and status[1, 1:3].tolist() == [1, 0]         # its second draw, slot 0
        for q in (0, 2):
            assert np.array_equal(targets[q], _reference(db, pools[q], draws[q], mus[q]))
        with pytest.raises(vqa.VqError) as group:
            db.batch_targets(pools, draws, mus)
        assert group.value.code == -1 and "query 1, draw 1: problem 0: singular system" in str(group.value)
        _check(db, [pools[0], pools[2]], [draws[0], draws[2]], [0.3, 0.0], what="after the refusal")
    finally:
        db.close()


def test_what_the_host_refuses(vqa):
    db = vqa.FeatureDB.from_arrays(_block(12, 1, 1, 68, "float32"))
    try:
        def refused(pools, draws, text, mus=None):
            with pytest.raises(vqa.VqError) as e:
                db.batch_targets(pools, draws, mus or [0.3] * len(pools))
            assert e.value.code == -1 and text in str(e.value), str(e.value)
        good = ((V, I), [([0, 1], [0])])
        refused([good[0], ([0, 12], [])], [good[1], [([0], [])]], "query 1: pool row 12 outside [0,12)")
        refused([good[0], ([-1], [])], [good[1], [([0], [])]], "pool row -1 outside")
        refused([([], I)], [[([], [0])]], "at least one validated match")
        refused([good[0]], [[([], [0, 1])]], "a draw needs a match")
        refused([good[0]], [[([0, 4], [0])]], "position 4 is a non-match of the pool, listed among the draw's matches")
        refused([good[0]], [[([0], [3])]], "position 7 outside its pool of 7 rows")
        refused([good[0]], [[([0, 2, 0], [1])]], "position 0 twice")
        refused([good[0]], [[([0], [-4])]], "listed among the draw's non-matches")
        refused([good[0]], [[]], "n_draws")
        refused([good[0]], [[([0], [])] * 65], "1 to 64 draws")
        refused([(list(range(12)) * 21 + [0, 1, 2, 3, 4], [])], [[([0], [])]], "n_pool_rows")
        refused([good[0]] * 17, [good[1]] * 17, "n_queries")
        off = (C.c_int64 * 11)()
        vqa._lib.call("vq_db_batch_targets_layout", db._h, 1, 7, 1, 3, off)
        buf = np.zeros(int(off[9]), dtype=np.uint8)
        with pytest.raises(vqa.VqError) as e:
            vqa._lib.call("vq_db_batch_targets", db._h, 1, 7, 1, 3, C.c_void_p(buf.ctypes.data), int(off[9]) - 1)
        assert "needs %d bytes" % off[9] in str(e.value)
        # a maximal layout on a real handle: the two [Q][S][E][D] pieces have their room too, the target piece is the last one
        vqa._lib.call("vq_db_batch_targets_layout", db._h, 16, 16 * 256, 16 * 64, 16 * 64 * 256, off)
        o = list(off)
        assert o[:10] == sorted(o[:10]) and all(v % 64 == 0 for v in o[:10])
        assert o[7] - o[6] >= 16 * 68 * 8 and o[9] - o[8] >= 16 * 68 * 8 and o[8] - o[7] >= 16 * 16
        _check(db, [good[0]], [good[1]], [0.3], what="after the refusals")
    finally:
        db.close()


def test_the_handles_other_state_is_left_alone(vqa):
    """A one-query round and a batched round first; batch_targets then changes neither the scores, nor the lists the batched round
    serves, nor the view in use -- and its rows are database rows whatever that view is."""
    x = _block(40, 2, 3, 256, "float32")
    db = vqa.FeatureDB.from_arrays(x)
    try:
        rng = np.random.default_rng(3)
        t = rng.standard_normal((3, 2, 3, 256)) * 1e-3
        w = np.array([[1.0, 1.5], [1.0, 0.5], [2.0, 1.0]])
        db.query_round(t[0], w[0], (0.0, -1e30))
        rounds = db.query_round_batch(t, w, selects=[(0.0, -1e30)] * 3)
        kept = [(np.array(r.scores), np.array(r.match_rows), np.array(r.near_rows)) for r in rounds]
        scores = db.scores()

        def fetch(q, nm, nn):
            m, k = np.empty(nm, dtype=np.int64), np.empty(nn, dtype=np.int64)
            vqa._lib.call("vq_db_batch_round_fetch", db._h, q, C.c_void_p(m.ctypes.data) if nm else None, nm, C.c_void_p(k.ctypes.data) if nn else None, nn)
            return m, k

        def active():
            v, n = C.c_int32(), C.c_int64()
            vqa._lib.call("vq_db_rows_active", db._h, C.byref(v), C.byref(n))
            return v.value, n.value
        before = active()
        pools, draws = [([0, 15, 16, 39], [1, 33])], [[([0, 1, 2, 3], [0, 1]), ([2, 1], [1])]]
        whole = _check(db, pools, draws, [0.3], what="whole database")
        assert np.array_equal(db.scores(), scores) and active() == before == (-1, 40)
        for q, (sc, m, k) in enumerate(kept):
            got_m, got_k = fetch(q, m.size, k.size)
            assert np.array_equal(got_m, m) and np.array_equal(got_k, k) and m.size + k.size > 0
        # under a search set that does not even hold the validated rows
        db.define_search_rows(7, np.arange(2, 12))
        db.use_search_set(7)
        db.query_round(t[1], w[1], (0.0, -1e30))
        scores = db.scores()
        before = active()
        got = db.batch_targets(pools, draws, [0.3])
        assert np.array_equal(got[0], whole[0])
        assert np.array_equal(db.scores(), scores) and active() == before and before[1] == 10 and db.search_set_in_use == 7
    finally:
        db.close()


def test_compute_matches_with_batched_targets_equals_the_batched_pass(vqa):
    """Six tickets of ONE pass on synth_small: three that bag (a finalize ticket among them), one simple, one partial_update with a
    previous target, and a new query -- the adjustment mode is a hyperparameter, so the pass's target factory hands every ticket's
    target its own copy of the pass's hyperparameters with that ticket's mode."""
    import copy
    g = golden_json("synth_small.json")
    x = golden_npy("synth_small_x.npy").astype(np.float32)
    ids = np.asarray(g["clip_order"])
    recs = records_from_dense(x.astype(np.float64), ids, [1, 2, 3])
    judged = [{"video_clip": int(c), "user_match": v} for c, v in zip(ids[[3, 9, 20, 31, 40, 41, 50]], [True, True, False, True, None, False, True])]
    modes = {7: "bagging", 12: "bagging", 30: "bagging", 25: "partial_update", 44: "simple", 51: "bagging"}

    class Repo:
        url = "http://offline/"

        def __init__(self, pairs):
            self._pairs = pairs

        def get_status(self):
            return self

        def items(self):
            return list(self._pairs)

    def run(**kw):
        db = vqa.FeatureDB.from_arrays(x, clip_ids=ids)
        db.stream_names, db.slot_splits = list(STREAMS), [[1, 2, 3]] * 2
        rng = np.random.default_rng(5)
        prev = {st: {str(sp): (rng.standard_normal(x.shape[3]) * 1e-3).tolist() for sp in (1, 2, 3)} for st in STREAMS}

        def update(row, revise, previous=None):
            u = {"query_id": int(row), "video_id": 1, "ref_clip": 0, "ref_clip_id": int(ids[row]), "search_set": 1, "number_of_matches_to_review": 20,
                 "dynamic_target_adjustment": revise, "user_matches": {}, "records": [r for r in recs if r["video_clip_id"] == int(ids[row])],
                 "feature_db": db}
            if revise:
                marks = [dict(m, is_match=True) for m in judged]
                u.update(latest_query_result={"id": 5, "round": 1, "bootstrapped_target": previous}, match_list=judged, match_page_size=3,
                         matches=marks, user_matches={str(m["video_clip"]): m["user_match"] for m in judged if m["user_match"] is not None})
            return u
        pairs = [("revise", update(7, True)), ("revise", update(12, True)), ("new", update(30, False)), ("revise", update(25, True, prev)),
                 ("revise", update(44, True)), ("finalize", update(51, True))]
        made, calls = [], []
        real_init, real_call = vqa.Ticket.__init__, vqa.FeatureDB.batch_targets

        def spy(self, *a, **k):
            real_init(self, *a, **k)
            made.append(self)

        def counted(self, pools, *a, **k):
            calls.append(len(pools))
            return real_call(self, pools, *a, **k)

        def target_factory(ticket, hp):
            own = copy.copy(hp)
            own.bootstrap_type = modes[ticket.query_id]
            return vqa.TargetClip(ticket, own)
        vqa.Ticket.__init__, vqa.FeatureDB.batch_targets = spy, counted
        hp = vqa.Hyperparameter(DEFAULT_WEIGHTS, 0.8, 0.0, 0.35, 0.3, STREAMS, "global_pool", 0.6, 0.7, "bagging", 3)
        try:
            random.seed(a=SEED)
            vqa.compute_matches(Repo(pairs), hp, batch=True, target_factory=target_factory, **kw)
            after = random.random()
        finally:
            vqa.Ticket.__init__, vqa.FeatureDB.batch_targets = real_init, real_call
        out = [(tk.ledger, tk.target.target_features, list(tk.matches.items()) if isinstance(tk.matches, dict) else tk.matches) for tk in made]
        db.close()
        return out, dict(hp.weights), hp.threshold, after, calls

    got, want = run(batch_targets=True), run()
    assert got[4] == [5] and want[4] == []                       # the five bootstrapping tickets in ONE call; none on the parent's path
    assert len(got[0]) == 6 and got[1:4] == want[1:4]
    for q, (a, b) in enumerate(zip(got[0], want[0])):
        assert a[1] == b[1], "ticket %d: target_features differ" % q
        assert a[0] == b[0] and a[2] == b[2] and len(a[2]) > 0, "ticket %d" % q
    targets = [np.array([[t[1][st][sp] for sp in (1, 2, 3)] for st in STREAMS]) for t in got[0]]
    assert len({t.tobytes() for t in targets}) == 6              # six different targets: every mode and reference clip left its mark
