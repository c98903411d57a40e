"""GPU: a group's whole weight update in one call (include/vq_amd_round_update.h, FeatureDB.batch_round_update) against the pieces it
chains, on the same round: the surfaces of batch_round_fit (bit for bit), Hyperparameter._pick_exact of surface / L (==), the scores
and partitions of batch_round_rescore under the device's own weights and band (==), the host's band expressions over the returned
scores and the one-query select of a second database under that band; then compute_matches(batch=True, fit_weights="device") against
fit_weights=True on a resident FeatureDB."""
import ctypes as C

import numpy as np
import pytest

import _pick_cases as pc
import sim_oracle as so
import test_batch_tickets_gpu as base
from _search_set_cases import np_select, same_bits
from test_pick_exact import BOUND

pytestmark = pytest.mark.gpu
D, BALLAST, NEAR = 256, 0.3, 0.35
FAR, NANROW = 5, 9                          # a row of zeros (it scores exactly 0 against everything) and a row of NaNs
SETS = {"a": lambda n: sorted(set(range(3, n, 7)) | {FAR, NANROW} | set(refs())), "b": lambda n: list(range(2, n - 20))}


def refs():
    return [13 + 11 * q for q in range(16)]


_CACHE = {}


def data(n, e):
    """Rows of |normal| features where every reference clip has 24 relatives blended towards it (scores from ~0.6 up to ~1), the two
    special rows, and the 16 queries made from the reference clips."""
    if (n, e) not in _CACHE:
        rng = np.random.default_rng(n + e)
        x = np.abs(rng.standard_normal((n, 2, e, D), dtype=np.float32)) * np.array([3.8, 1.2], dtype=np.float32).reshape(1, 2, 1, 1)
        for k, ref in enumerate(refs()):
            rel = np.array([r for r in (ref + 1 + 3 * np.arange(24)) % n if r not in refs()])
            a = np.linspace(0.05, 0.98, len(rel), dtype=np.float32)[np.random.default_rng(k).permutation(len(rel))].reshape(-1, 1, 1, 1)
            x[rel] = a * x[ref] + (1 - a) * x[rel]
        x[FAR] = 0.0
        x[NANROW] = np.nan
        t = np.stack([np.stack([[so.scale_feature(x[r, s, k].astype(np.float64)) for k in range(e)] for s in range(2)]) for r in refs()])
        _CACHE[(n, e)] = (x, t)
    return _CACHE[(n, e)]


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    if base.X is None:
        base.X = base.features()
    return m


def pair(vqa, n, e, dtype, sets):
    x, t = data(n, e)
    out = []
    for _ in range(2):
        db = vqa.FeatureDB.from_arrays(x.astype(dtype), dtype=dtype)
        for sid in sorted(set(s for s in sets if s is not None)):
            db.define_search_rows(sid, np.array(SETS[sid](n), dtype=np.int64))
        out.append(db)
    return out[0], out[1], t


def run_round(db, t, Q, sets):
    w0 = np.array([[1.0, 0.6 + 0.1 * q] for q in range(Q)])
    bands0 = np.array([[0.8, 0.73]] * Q)
    if any(s is not None for s in sets):
        return db.query_round_batch_sets(t[:Q], w0, sets, bands0)
    return db.query_round_batch(t[:Q], w0, bands0)


def position(n, sid, row):
    """Where database row ``row`` stands in the view of search set ``sid``."""
    return row if sid is None else SETS[sid](n).index(row)


def member_inputs(n, sid, q, scores, L, mode, rng):
    """(rows, labels, reach, user_rows) of one member: L labelled positions -- the better half of the sample confirmed, one verdict in
    ten flipped -- and the user rows of its kind."""
    m = scores.shape[0]
    pool = np.argsort(-np.nan_to_num(scores, nan=-1.0))[:max(40, m // 4)] if L <= 64 else np.arange(m)
    rows = pool[rng.integers(0, len(pool), size=L)].astype(np.int64)
    rows[np.isnan(scores[rows])] = position(n, sid, refs()[q])                                 # the NaN row carries no label
    y = ((scores[rows] >= (np.median(scores[rows]) if L else 0.0)) ^ (rng.random(L) < 0.1)).astype(np.float64)
    own = position(n, sid, refs()[q])
    user = {"revise": None, "U0": [], "below": sorted([position(n, sid, FAR), own]), "above": [own],
            "nan": sorted([position(n, sid, NANROW), own, int(pool[3])])}[mode]
    return rows, y, (NEAR if mode == "revise" else None), user


def host_band(th, reach, scores, user, eps):
    """compute_matches._review_budget and the first line of select_clips_to_review, as the ticket evaluates them."""
    lowest = 1
    if reach is None:
        for r in sorted(user):
            lowest = min(lowest, scores[r])
        reach = max(th - lowest, 0) / max(1 - th, eps)
    return lowest, (float(th), float(th - reach * (1 - th)))


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


def poison_round_block(db, Q, views):
    """The next block a call on the last round takes from its pool holds 0xA5 in every byte."""
    last = db._bround_last
    assert last.Q == Q and last.views == views
    blk = last.block(db.blocks)                                # the route of the call itself
    blk.bytes()[:] = 0xA5
    del blk                                                    # back into its pool, on top


# (N, E, dtype, the search set of each query (None: the whole database), [(query, L, kind of member)]); every other query of the round
# is outside the update, a member with L = 0 is a slot that is skipped
CASES = {
    "n200-e1-f32-q1": (200, 1, np.float32, [None], [(0, 7, "below")]),
    "n200-e2-f16-q3": (200, 2, np.float16, [None] * 3, [(0, 1, "above"), (1, 0, "revise"), (2, 7, "nan")]),
    "n4200-e2-f32-q16": (4200, 2, np.float32, [None] * 16, [(0, 7, "revise"), (1, 4097, "below"), (2, 1, "U0"), (4, 20, "above"), (5, 0, "U0"),
                                                           (6, 7, "nan"), (7, 33, "revise"), (15, 60, "below")]),
    "n4200-e1-f16-q16-all": (4200, 1, np.float16, [None] * 16, [(q, 5 + q, ("revise", "above", "below", "nan")[q % 4]) for q in range(16)]),
    "n4200-e1-f32-views-q3": (4200, 1, np.float32, ["a", None, "b"], [(0, 7, "below"), (1, 4097, "revise"), (2, 20, "above")]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_equals_fit_pick_rescore_band_and_select(vqa, case):
    n, e, dtype, sets, members = CASES[case]
    Q, views = len(sets), any(s is not None for s in sets)
    db, ref, t = pair(vqa, n, e, dtype, sets)
    results = run_round(db, t, Q, sets)
    before = [(np.array(r.scores), np.array(r.match_rows), np.array(r.near_rows), r.near_argmax) for r in results]
    hp = pc.make_hp(vqa)
    cand, ths, eps = pc.candidates(hp), np.asarray(hp.threshold_grid, dtype=np.float64), pc.compute_eps()
    rng = np.random.default_rng(17)
    queries = [q for q, _L, _mode in members]
    inputs = [member_inputs(n, sets[q], q, before[q][0], L, mode, rng) for q, L, mode in members]
    k = len(members)
    served = [i for i in range(k) if members[i][1] > 0]
    want_surfaces = db.batch_round_fit([queries[i] for i in served], [inputs[i][0] for i in served], [inputs[i][1] for i in served],
                                       [cand] * len(served), [ths] * len(served), [BALLAST] * len(served))
    want_surfaces = {i: np.array(s) for i, s in zip(served, want_surfaces)}
    poison_round_block(db, Q, views)
    got = db.batch_round_update(queries, [x[0] for x in inputs], [x[1] for x in inputs], [cand] * k, [ths] * k, [BALLAST] * k, [1] * k, eps,
                                [x[2] for x in inputs], [x[3] for x in inputs], want_surface=True)
    raw = got[served[0]].scores.base                           # the block of the round the call wrote into
    off, start = db._bround_last.off, db._bround_last.start
    assert raw.dtype == np.uint8 and raw.shape[0] >= off[9]
    weights, bands = [], []
    for i in served:
        q, L, mode = members[i]
        r = got[i]
        # 1. the surface is the fit's
        assert same_bits(r.surface, want_surfaces[i]), (q, L)
        # 2. the pick is _pick_exact's of surface / L
        want = pc.exact_pick(hp, want_surfaces[i], L)
        assert pc.same_pick((float(r.w), float(r.threshold), r.iw, r.it, r.on_rim, r.fell_back), want), (q, L, want)
        w = np.array(cand[r.iw])
        w[1] = r.w
        weights.append(w)
        bands.append(r.band)
        # 4. lowest and band are the host's expressions over the returned scores
        rows, y, reach, user = inputs[i]
        lowest, band = host_band(r.threshold, reach, r.scores, user or [], eps)
        print(case, q, L, mode, "pick", want, "lowest", float(r.lowest), "band", r.band, "lists", len(r.match_rows), len(r.near_rows))
        assert float(r.lowest) == float(lowest) and r.band == band, (q, mode, r.lowest, lowest, r.band, band)
        th = float(r.threshold)
        if mode == "below":
            assert r.lowest == 0.0 < th and r.band[1] <= 1e-12
        elif mode == "above":
            assert th <= r.lowest < 1.0 + 1e-9 and r.band[1] == th
        elif mode == "nan":
            assert np.isnan(r.scores[position(n, sets[q], NANROW)]) and np.isfinite(r.lowest) and r.lowest < 1.0
        elif mode == "U0":
            assert r.lowest == 1.0 and r.band[1] == th
        # ... and the lists are the one-query select's under that band, on a second database with the same similarities
        if sets[q] is not None or views:
            ref.use_search_set(sets[q])
        ref.write_avg(np.array(r.avg), np.array(r.n_e))
        ref.rescore(w)
        assert same_bits(r.scores, ref.scores()), q
        m_rows, k_rows, am = ref.select(*r.band)
        assert np.array_equal(r.match_rows, m_rows) and np.array_equal(r.near_rows, k_rows) and r.near_argmax == am, (q, mode)
        fm, fk = fetch(vqa, db, q, len(m_rows), len(k_rows))
        assert np.array_equal(fm, m_rows) and np.array_equal(fk, k_rows)
        assert r.avg is results[q].avg and r.n_e is results[q].n_e
    # slots with L = 0 and queries outside the update: nothing of theirs was written, in the block, in the lists or on the device
    P = off[10]
    sc_raw = raw[off[5]:off[5] + start[Q] * 8]
    res_raw = raw[off[6]:off[6] + Q * 32].reshape(Q, 32)
    pre_raw = [raw[off[p]:off[p] + Q * P * 8].reshape(Q, P * 8) for p in (7, 8)]
    assert (raw[:off[5]] == 0xA5).all()                                                        # queries, weights, bands, n_e, avg: never written
    touched = {queries[i] for i in served}
    for i in range(k):
        if i not in served:
            assert got[i].scores is None and got[i].match_rows is None and got[i].w is None and got[i].surface is None
    for q in range(Q):
        if q in touched:
            continue
        assert (sc_raw[start[q] * 8:start[q + 1] * 8] == 0xA5).all() and (res_raw[q] == 0xA5).all(), q
        assert (pre_raw[0][q] == 0xA5).all() and (pre_raw[1][q] == 0xA5).all(), q
        sc, m_rows, k_rows, am = before[q]
        fm, fk = fetch(vqa, db, q, len(m_rows), len(k_rows))
        assert np.array_equal(fm, m_rows) and np.array_equal(fk, k_rows), q
    if not views:
        dev = device_scores(vqa, db, Q, n)
        for q in range(Q):
            assert same_bits(dev[q], np.array(got[queries.index(q)].scores) if q in touched else before[q][0]), q
    # 3. scores and partitions are those of batch_round_rescore under the device's own weights and band, on the same round
    again = db.batch_round_rescore([queries[i] for i in served], np.stack(weights), np.array(bands))
    for i, r2 in zip(served, again):
        r = got[i]
        assert same_bits(r.scores, r2.scores) and np.array_equal(r.match_rows, r2.match_rows) and np.array_equal(r.near_rows, r2.near_rows)
        assert r.near_argmax == r2.near_argmax
    db.close()
    ref.close()


def test_given_surfaces_are_picked_like_pick_exact(vqa):
    """The crafted surfaces of tests/_pick_cases.py go up instead of the fit (rows and labels empty, L still the divisor): every pick
    == _pick_exact -- rims and corners, ties (the first in row-major order, also ties the division creates), the first NaN, inf cells,
    1e300, the all-equal surface (cell (0, 0), on the rim) -- and scores and lists follow the picked weights and band."""
    db, ref, t = pair(vqa, 200, 1, np.float32, [None])
    results = run_round(db, t, 16, [None] * 16)
    hp = pc.make_hp(vqa)
    cand, ths, eps = pc.candidates(hp), np.asarray(hp.threshold_grid, dtype=np.float64), pc.compute_eps()
    crafted = sorted(pc.crafted_surfaces().items())
    assert len(crafted) > 16 and "all-equal" in dict(crafted)
    for chunk in (crafted[:16], crafted[16:]):
        k = len(chunk)
        queries = list(range(16 - k, 16))                                                      # the second call: a run that starts inside the round
        reaches = [None if i == 1 else NEAR for i in range(k)]
        got = db.batch_round_update(queries, [None] * k, [L for _name, (_s, L) in chunk], [cand] * k, [ths] * k, [BALLAST] * k, [1] * k, eps,
                                    reaches, [[]] * k, surfaces=[s for _name, (s, _L) in chunk])
        for (name, (surface, L)), r, q, reach in zip(chunk, got, queries, reaches):
            want = pc.exact_pick(hp, surface, L)
            assert pc.same_pick((float(r.w), float(r.threshold), r.iw, r.it, r.on_rim, r.fell_back), want), (name, want)
            assert r.surface is None and r.lowest == 1.0
            w = np.array(cand[r.iw])
            w[1] = r.w
            ref.write_avg(np.array(results[q].avg), np.array(results[q].n_e))
            ref.rescore(w)
            assert same_bits(r.scores, ref.scores()), name
            lowest, band = host_band(r.threshold, reach, r.scores, [], eps)
            assert np.array_equal(np.array(r.band), np.array(band), equal_nan=True), (name, r.band, band)
            m_rows, k_rows, am = np_select(np.array(r.scores), *r.band)
            assert np.array_equal(r.match_rows, m_rows) and np.array_equal(r.near_rows, k_rows) and r.near_argmax == am, name
            if name == "all-equal":
                assert (r.iw, r.it, r.on_rim, r.fell_back) == (0, 0, True, False)
    db.close()
    ref.close()


def test_refusals_are_argument_checks_and_leave_the_round_usable(vqa, monkeypatch):
    db, ref, t = pair(vqa, 200, 1, np.float32, [None])
    hp = pc.make_hp(vqa)
    cand, ths, eps = pc.candidates(hp), np.asarray(hp.threshold_grid, dtype=np.float64), pc.compute_eps()
    rows, y = np.array([20, 31, 199], dtype=np.int64), np.array([1.0, 0.0, 1.0])

    def update(q=1, rows=rows, y=y, cand=cand, ths=ths, second=1, reach=NEAR, user=(), **kw):
        return db.batch_round_update([q], [rows], [y], [cand], [ths], [BALLAST], [second], eps, [reach], [list(user)], **kw)

    def refused(code, **kw):
        with pytest.raises(vqa.VqError) as ei:
            update(**kw)
        assert ei.value.code == code, str(ei.value)
    refused(-4)                                                                                # no batched round yet
    results = run_round(db, t, 3, [None] * 3)
    kept = [np.array(r.scores) for r in results]
    refused(-4, q=3)                                                                           # a query the round did not have
    refused(-1, rows=np.array([20, 31, 200]))                                                  # a row = M_q
    refused(-1, rows=np.array([-1, 31, 199]))
    refused(-1, reach=None, user=[200])                                                        # a user row = M_q
    refused(-1, reach=None, user=[-1])
    refused(-1, second=2)                                                                      # S = 2
    refused(-1, second=-1)
    refused(-1, cand=np.ones((65, 2)))                                                         # G = 65
    refused(-1, ths=np.linspace(0.5, 1.0, 65))                                                 # T = 65
    import sys
    fdb = sys.modules[vqa.FeatureDB.batch_round_update.__module__]
    real = fdb.call

    def short_round_block(name, *a):
        if name == "vq_db_batch_round_update":
            a = a[:9] + (a[9] - 64,) + a[10:]
        return real(name, *a)
    monkeypatch.setattr(fdb, "call", short_round_block)
    refused(-1)                                                                                # a short block of the round
    monkeypatch.setattr(fdb, "call", real)
    # nothing was launched: the device still holds the round's scores, and the update then works
    dev = device_scores(vqa, db, 3, 200)
    assert all(same_bits(dev[q], kept[q]) for q in range(3))
    surface = np.array(db.batch_round_fit([1], [rows], [y], [cand], [ths], [BALLAST])[0])
    r = update(want_surface=True)[0]
    assert same_bits(r.surface, surface)
    assert pc.same_pick((float(r.w), float(r.threshold), r.iw, r.it, r.on_rim, r.fell_back), pc.exact_pick(hp, surface, 3))
    quiet = update(want_scores=False)[0]                                                       # the scores stay on the device
    assert quiet.scores is None and np.array_equal(quiet.match_rows, r.match_rows) and quiet.band == r.band
    assert same_bits(device_scores(vqa, db, 3, 200)[1], np.array(r.scores))
    db.close()
    ref.close()


def test_compute_matches_with_the_update_on_the_device(vqa):
    """compute_matches(batch=True, fit_weights="device") on a resident FeatureDB against fit_weights=True on a second one: one pass and
    ONE update call, no fit, rescore, write_avg or select behind it (the finalize ticket's band came from the device).  Every weight
    lies within the bound of tests/test_pick_exact.py of _pick_from's; with these labels the picks agree bit for bit (asserted), and so
    ledger and matches are identical."""
    import test_batch_fit_tickets_gpu as ft
    dbs = [base.resident(vqa) for _ in range(2)]
    updates = []
    real = type(dbs[0]).batch_round_update

    def counted(self, *a, **kw):
        updates.append(list(a[0]))
        return real(self, *a, **kw)
    type(dbs[0]).batch_round_update = counted
    try:
        dev = ft.run(vqa, dbs[0], ft.updates(dbs[0]), batch=True, fit_weights="device")
    finally:
        type(dbs[0]).batch_round_update = real
    fit = ft.run(vqa, dbs[1], ft.updates(dbs[1]), batch=True, fit_weights=True)
    assert dev[3] == ["query_round_batch"] and updates == [[3, 4, 5, 6]]
    assert fit[3] == ["query_round_batch", "batch_round_fit", "batch_round_rescore", "write_avg", "rescore", "select"]
    made_d, hp_d = dev[0], dev[1]
    made_f, hp_f = fit[0], fit[1]
    assert [tk.ledger["process_state"] for tk in made_d] == [tk.ledger["process_state"] for tk in made_f] == [[3, 4]] * 4 + [[3, 7]] + [[3, 4]] * 2
    agree = True
    for a, b in zip(made_d, made_f):
        assert (a._fit is None) == (b._fit is None)
        if a._fit is None:
            continue
        got = np.array([a._fit[0]["warped_optical_flow"], a._fit[1]])
        want = np.array([b._fit[0]["warped_optical_flow"], b._fit[1]])
        rel = np.abs(got - want) / np.abs(want)
        print(a.query_id, "fit", got, "relative difference to _pick_from's", rel)
        assert (rel <= BOUND).all(), (a.query_id, rel)
        agree = agree and bool((rel == 0).all())
    # these labels: every pick of _pick_exact has _pick_from's bits (two on the rim, two refined), so the runs are identical
    assert agree and ft.outcome(made_d, hp_d) == ft.outcome(made_f, hp_f)
    assert all(len(tk.matches) > 0 for tk in made_d)
    for db in dbs:
        db.close()


def test_close_frees_the_update_blocks(vqa):
    """The page-locked blocks of batch_round_update go with the database: close() empties their pool and marks it closed, so a block
    still held by a result is freed, not pooled, when its last view goes (the free function of the registry is counted)."""
    db, ref, t = pair(vqa, 200, 1, np.float32, [None])
    ref.close()
    run_round(db, t, 3, [None] * 3)
    hp = pc.make_hp(vqa)
    cand, ths = pc.candidates(hp), np.asarray(hp.threshold_grid, dtype=np.float64)
    args = ([1], [np.array([20, 31, 199])], [np.array([1.0, 0.0, 1.0])], [cand], [ths], [BALLAST], [1], pc.compute_eps(), [NEAR], [[]])
    held = db.batch_round_update(*args, want_surface=True)[0]                                   # its block is held by the surface
    db.batch_round_update(*args)                                                               # this one's is idle in the pool by now
    blocks, freed = db.blocks, []
    real_free = blocks._free
    blocks._free = lambda ptr: (freed.append(ptr), real_free(ptr))
    idle = [ptr for ptr, _size in blocks.idle("update")]
    assert len(idle) >= 1 and not blocks.closed
    db.close()
    assert blocks.closed and not blocks.idle("update") and set(idle) <= set(freed)
    ptr = held.surface.base.base.ptr                                                           # the update block the surface is a view of
    assert ptr not in freed and ptr not in idle
    del held
    assert freed.count(ptr) == 1                                                               # freed when released ...
    assert not blocks.idle("update")                                                           # ... and not pooled
