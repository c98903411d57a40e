"""GPU: batched query rounds (include/vq_amd_rounds.h, FeatureDB.query_round_batch) -- up to 16 rounds in one read of the database,
against the one-query calls on the same handle, oracle/sim_oracle.py run once per query and a numpy stable partition."""
import ctypes as C
import threading

import numpy as np
import pytest

import sim_oracle as so
from _search_set_cases import np_select, round_layout, same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-12           # what tests/test_sim_gpu.py holds the batched pass to


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
    """Missing splits, every (clip, stream) keeping at least one (no NaN averages to compare)."""
    present = np.ones((n, s, e), dtype=np.uint8)
    present[::7, 0, 0] = 0
    present[3::11, s - 1, e - 1] = 0
    present[n - 1, :, 0] = 0
    present[..., 0] |= (present.sum(axis=2) == 0).astype(np.uint8)
    return present


def _partition(v, th, lower):
    """numpy stable partition and first arg-max of the near band (ticket.py:325-340)."""
    match = np.flatnonzero(v >= th)
    near = np.flatnonzero((lower <= v) & (v < th))
    return match, near, (int(near[np.argmax(v[near])]) if near.size else -1)


def _check_partitions(results, bands):
    for q, r in enumerate(results):
        match, near, am = _partition(r.scores, bands[q, 0], bands[q, 1])
        assert r.match_rows.dtype == np.int64 and r.near_rows.dtype == np.int64
        assert len(r.match_rows) == len(match) and len(r.near_rows) == len(near), q          # the counts
        assert (r.match_rows == match).all() and (r.near_rows == near).all(), q
        assert r.near_argmax == am, q


# (dtype, Q, n, S, E, D, mask, layout).  The issue's table, with one correction: it asks for the tiled layout at D = 768 / S = 3 and at
# D = 256, shapes vq_db_set_layout refuses (tiled holds fp32, D = 1024, S <= 2, E <= 5: tests/test_sim_gpu.py pins the refusal).  Those
# two shapes run in the layout the library can hold them in, and two tiled cases at D = 1024 are ADDED for what the table wanted from
# them: the tiled branch with a mask at n = 4 100, and the three-pass selection just past kSelSmallN = 16 384 on a tiled database.
CASES = [
    (np.float32, 1, 16, 1, 1, 256, False, "rows"),            # one tile, one slot in use
    (np.float32, 16, 33, 2, 5, 1024, False, "rows"),          # ragged tile, all slots
    (np.float64, 5, 700, 2, 3, 1024, True, "rows"),           # unused query slots, missing splits
    (np.float16, 16, 1003, 2, 3, 1024, True, "rows"),         # fp16 ring
    (np.float32, 9, 4100, 3, 2, 768, True, "rows"),           # 3 streams, D = 768 (the table says tiled: refused for this shape)
    (np.float32, 16, 16_400, 2, 1, 256, False, "rows"),       # just past kSelSmallN: the three-pass selection (table: tiled, refused)
    (np.float32, 16, 140_007, 2, 1, 256, True, "rows"),       # second round of tiles (> 256 x 16 x 2 x 16 clips)
    (np.float32, 9, 4100, 2, 2, 1024, True, "tiled"),         # added: the tiled branch, masked, fetch path
    (np.float32, 16, 16_400, 2, 1, 1024, False, "tiled"),     # added: tiled and the three-pass selection
    # the kernels of VQ_FUSED_LAUNCH the cases above do not launch (every case runs the plain pass, scan_batch, and the round form)
    (np.float64, 16, 1003, 2, 1, 256, True, "rows"),
    (np.float64, 7, 700, 1, 2, 512, False, "rows"),
    (np.float64, 9, 1003, 3, 2, 768, True, "rows"),
    (np.float16, 16, 1003, 1, 2, 512, True, "rows"),
    (np.float16, 9, 1003, 3, 2, 768, False, "rows"),          # fp16, D = 768: the 2-buffer ring, NCHUNK = 6
    (np.float16, 16, 131_155, 2, 1, 256, True, "rows"),       # a short second round of tiles (n > 512 clips per compute unit)
    (np.float64, 16, 131_155, 2, 1, 256, False, "rows"),      # the same on fp64 rows
    (np.float32, 5, 203, 2, 2, 512, False, "rows"),
    (np.float32, 5, 203, 2, 2, 512, True, "rows"),
    (np.float32, 5, 203, 1, 3, 768, False, "rows"),
    (np.float32, 5, 203, 2, 2, 1024, True, "rows"),
    (np.float64, 5, 203, 2, 2, 512, True, "rows"),
    (np.float64, 5, 203, 1, 3, 768, False, "rows"),
    (np.float64, 5, 203, 2, 2, 1024, False, "rows"),
    (np.float16, 5, 203, 2, 2, 256, False, "rows"),
    (np.float16, 5, 203, 2, 2, 512, False, "rows"),
    (np.float16, 5, 203, 1, 3, 768, True, "rows"),
    (np.float16, 5, 203, 2, 2, 1024, False, "rows"),
]
# Coverage of the 24 row-major kernels batch_fused_kernel<T, D / 256, 2, masked, 8> (and of their round forms) by the "rows" cases
# above, as n of a case that launches it -- a new storage type or width in VQ_FUSED_LAUNCH gets new cases and a new row here:
#
#   dtype    D = 256            D = 512           D = 768           D = 1024
#   f16      203 / 131 155 m    203 / 1 003 m     1 003 / 203 m     203 / 1 003 m         (plain / m = with a presence mask)
#   f32      16 / 140 007 m     203 / 203 m       203 / 4 100 m     33 / 203 m
#   f64      131 155 / 1 003 m  700 / 203 m       203 / 1 003 m     203 / 700 m
ROW_MAJOR_KERNELS = {(dt, d, m) for dt in (np.float16, np.float32, np.float64) for d in (256, 512, 768, 1024) for m in (False, True)}
assert ROW_MAJOR_KERNELS == {(c[0], c[5], c[6]) for c in CASES if c[7] == "rows"}


@pytest.mark.parametrize("dtype,Q,n,S,E,D,mask,layout", CASES)
def test_batched_round_against_single_rounds_oracle_and_numpy_partition(vqa, cus, dtype, Q, n, S, E, D, mask, layout):
    """Per case: scores == scan_batch bit for bit; avg <= 1e-12 from the one-query scan and from the oracle; n_e exact;
    dense_scores(avg, w) <= 1e-12 from the scores; match / near lists, counts and near_argmax == the numpy stable partition of the
    RETURNED scores, exactly; a second call returns the same bits.  Bands come from quantiles of each query's scores; special
    queries: threshold above the maximum with two equal largest near scores (a clip duplicated through upload: the first wins),
    lower == threshold (no near list), and at n >= 4100 a threshold below the minimum (all n rows match: the fetch path)."""
    if n > 131_072:
        assert n > cus * 512                                   # a workgroup per compute unit takes 16 waves x 2 tiles x 16 clips per round
    x = _features(n, S, E, D, dtype, seed=n + Q)
    r0, dup = min(7, n - 1), n - 3                             # query 0 is made from clip r0; row dup becomes a copy of it
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
    rng = np.random.default_rng(Q * 1000 + n)
    targets = rng.standard_normal((Q, S, E, D)) / D
    targets[0] = np.stack([[so.scale_feature(x[r0, s, e].astype(np.float64)) for e in range(E)] for s in range(S)])
    weights = 0.5 + rng.random((Q, S))
    want_scores = db.scan_batch(targets, weights)
    bands = np.empty((Q, 2))
    for q in range(Q):
        lo, hi = np.quantile(want_scores[q], [0.90, 0.97])
        bands[q] = (hi, lo)
    bands[0] = (2.0, np.quantile(want_scores[0], 0.5))        # above the maximum: no match; the two copies of r0 are the largest near scores
    if Q > 1:
        bands[1, 1] = bands[1, 0]                             # lower == threshold: no near list
    if Q > 2 and n >= 4100:
        bands[2] = (want_scores[2].min() - 1.0, want_scores[2].min() - 2.0)      # everything matches: longer than the prefix

    off = (C.c_int64 * 12)()
    vqa._lib.call("vq_db_batch_round_layout", db._h, Q, off)
    assert list(off) == round_layout(Q, S, E, D, n=n)[0]
    got = db.query_round_batch(targets, weights, bands)
    assert len(got) == Q
    for q, r in enumerate(got):
        assert r.scores.shape == (n,) and r.avg.shape == (n, S) and r.n_e is got[0].n_e
        assert (r.scores == want_scores[q]).all(), q                                          # bit for bit
    _check_partitions(got, bands)
    # the special queries did what they were made for
    assert len(got[0].match_rows) == 0 and got[0].near_argmax == min(r0, dup) and got[0].scores[r0] == got[0].scores[dup]
    assert got[0].scores[r0] == got[0].scores[got[0].near_rows].max()
    if Q > 1:
        assert len(got[1].near_rows) == 0 and got[1].near_argmax == -1 and len(got[1].match_rows) > 0
    else:
        alone = db.query_round_batch(targets, weights, np.array([[bands[0, 1], bands[0, 1]]]))
        _check_partitions(alone, np.array([[bands[0, 1], bands[0, 1]]]))
        assert len(alone[0].near_rows) == 0 and alone[0].near_argmax == -1 and len(alone[0].match_rows) > 0
    if Q > 2 and n >= 4100:
        assert len(got[2].match_rows) == n > 1024 and (got[2].match_rows == np.arange(n)).all()
    for q in range(3, Q):
        assert len(got[q].match_rows) > 0 and len(got[q].near_rows) > 0                       # quantile bands: both lists non-empty
    # against the one-query scan on the same handle and the oracle
    xo = x.astype(np.float64)
    for q in range(Q):
        db.set_query(targets[q])
        db.scan(weights[q])
        avg1, ne1 = db.similarities()
        assert (got[q].n_e == ne1).all()
        assert np.abs(got[q].avg - avg1).max() <= TOL, q
        assert np.abs(got[q].scores - db.scores()).max() <= TOL, q
        _, o_avg, o_ne = so.dense_similarities(xo, targets[q], present)
        assert (got[q].n_e == o_ne).all()
        assert np.abs(got[q].avg - o_avg).max() <= TOL, q
        assert np.abs(got[q].scores - so.dense_scores(o_avg, weights[q])).max() <= TOL, q
        assert np.abs(so.dense_scores(got[q].avg, weights[q]) - got[q].scores).max() <= TOL, q
    again = db.query_round_batch(targets, weights, bands)
    for a, b in zip(got, again):
        assert (a.scores == b.scores).all() and (a.avg == b.avg).all() and (a.n_e == b.n_e).all()
        assert (a.match_rows == b.match_rows).all() and (a.near_rows == b.near_rows).all() and a.near_argmax == b.near_argmax
    db.close()


def _small_db(vqa, n=700, seed=5):
    x = so.cfg1_features(n=n, e=3, seed=seed)
    present = np.ones((n, 2, 3), dtype=np.uint8)
    present[5, 0, 2] = 0
    present[n // 6, 1, :2] = 0
    db = vqa.FeatureDB.from_arrays(x, present=present)
    rows = [(7 + 41 * i) % n for i in range(6)]
    targets = np.stack([np.stack([[so.scale_feature(x[r, s, e].astype(np.float64)) for e in range(3)] for s in range(2)]) for r in rows])
    weights = np.stack([[1.0, 1.5 + 0.1 * i] for i in range(6)])
    return db, x, targets, weights


def test_a_batched_round_leaves_the_one_query_state_alone(vqa):
    """set_query / scan(w) / select on a handle, then a batched round: scores, similarities and the select_fetch lists read back
    identical, and a re-weighting of the handle's similarities is still the first query's."""
    db, _x, targets, weights = _small_db(vqa)
    db.set_query(targets[0])
    db.scan(weights[0])
    scores = db.scores()
    avg, ne = db.similarities()
    lo, hi = np.quantile(scores, [0.5, 0.9])
    nm, nn, am = C.c_int64(), C.c_int64(), C.c_int64()
    vqa._lib.call("vq_db_select", db._h, float(hi), float(lo), C.byref(nm), C.byref(nn), C.byref(am))

    def fetch():
        m, k = np.empty(nm.value, dtype=np.int64), np.empty(nn.value, dtype=np.int64)
        vqa._lib.call("vq_db_select_fetch", db._h, m.ctypes.data_as(C.c_void_p), m.size, k.ctypes.data_as(C.c_void_p), k.size)
        return m, k
    m0, k0 = fetch()
    assert nm.value > 0 and nn.value > 0
    bands = np.tile([[0.3, 0.1]], (5, 1))
    got = db.query_round_batch(targets[1:], weights[1:], bands)
    assert all(len(r.match_rows) + len(r.near_rows) > 0 for r in got)
    assert (db.scores() == scores).all()
    avg2, ne2 = db.similarities()
    assert (avg2 == avg).all() and (ne2 == ne).all()
    m1, k1 = fetch()
    assert (m1 == m0).all() and (k1 == k0).all()
    db.rescore(weights[3])
    assert (db.scores() == so.dense_scores(avg, weights[3])).all()
    db.close()


def test_refusals(vqa):
    db, x, targets, weights = _small_db(vqa, n=100)
    with pytest.raises(vqa.VqError):
        db.query_round_batch(targets[:0], weights[:0], None)                                  # Q = 0
    with pytest.raises(vqa.VqError):
        db.query_round_batch(np.zeros((17, 2, 3, 1024)), np.ones((17, 2)), None)              # Q = 17
    db.define_search_rows("some", np.arange(10, 60))
    db.use_search_set("some")
    with pytest.raises(vqa.VqError) as ei:
        db.query_round_batch(targets[:2], weights[:2], None)                                  # a search set in use
    assert ei.value.code == -5 and "whole database" in str(ei.value)
    db.use_search_set(None)
    assert len(db.query_round_batch(targets[:2], weights[:2], None)) == 2
    # a block that is too small, and an unknown flag bit, at the ctypes level
    off = (C.c_int64 * 12)()
    vqa._lib.call("vq_db_batch_round_layout", db._h, 2, off)
    assert all(int(v) % 64 == 0 for v in off[:10]) and off[10] == 1024
    p = C.c_void_p()
    vqa._lib.call("vq_host_alloc", C.byref(p), int(off[9]))
    lib = vqa.load_library()
    assert lib.vq_db_query_round_batch(db._h, 2, p, int(off[9]) - 1, 7) == -1
    assert lib.vq_db_query_round_batch(db._h, 2, p, int(off[9]), 16) == -1
    assert lib.vq_db_batch_round_fetch(db._h, 5, None, 0, None, 0) == -4                     # the last round had 2 queries
    vqa._lib.call("vq_host_free", p)
    db.close()
    odd = vqa.FeatureDB.synthetic(50, 2, 1, 260, seed=3)
    with pytest.raises(vqa.VqError):
        odd.query_round_batch(np.zeros((2, 2, 1, 260)), np.ones((2, 2)), None)                # D = 260
    odd.close()


def test_one_query_rounds_and_batched_rounds_from_two_threads(vqa):
    """One thread loops query_round, the other query_round_batch, on ONE handle: each gets its serial results."""
    db, _x, targets, weights = _small_db(vqa)
    bands = np.tile([[0.3, 0.1]], (5, 1))
    serial_one = db.query_round(targets[0], weights[0], (0.3, 0.1))
    serial_one = [np.array(a) for a in (serial_one.avg, serial_one.scores, serial_one.match_rows, serial_one.near_rows)] + [serial_one.near_argmax]
    serial_b = [([np.array(a) for a in (r.avg, r.scores, r.match_rows, r.near_rows)] + [r.near_argmax]) for r in db.query_round_batch(targets[1:], weights[1:], bands)]
    errors = []

    def same(a, b):
        return all((x == y).all() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]

    def one():
        try:
            for _ in range(6):
                r = db.query_round(targets[0], weights[0], (0.3, 0.1))
                assert same([r.avg, r.scores, r.match_rows, r.near_rows, r.near_argmax], serial_one)
        except BaseException as e:                            # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    def many():
        try:
            for _ in range(6):
                for r, want in zip(db.query_round_batch(targets[1:], weights[1:], bands), serial_b):
                    assert same([r.avg, r.scores, r.match_rows, r.near_rows, r.near_argmax], want)
        except BaseException as e:                            # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=one), threading.Thread(target=many)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    db.close()


# ---------------------------------------------------------------------------------------------------------------- awkward inputs
# fp32, S = 2, E = 3, D = 256, Q = 5 on both sides of kSelSmallN = 16 384: the one-workgroup selection and the three-pass one, with the
# last size of the first (16 384) and the first size of the second (16 385: nine blocks, the last holding one row)
AWKWARD_N = [700, 16_384, 16_385, 16_400]


def _lost_rows(n):
    """rows that lose every split of one stream (2 047 | 2 048: the edge of a selection chunk)"""
    return [0, 5, n - 1] + ([2047, 2048] if n > 2048 else [])


def _awkward_db(vqa, n, lose):
    S, E, D, Q = 2, 3, 256, 5
    x = _features(n, S, E, D, np.float32, seed=n + 1)
    present = _mask(n, S, E)
    lost = {r: i % S for i, r in enumerate(_lost_rows(n))} if lose else {}
    for r, s in lost.items():
        present[r, s, :] = 0
    db = vqa.FeatureDB.from_arrays(x, present=present)
    rng = np.random.default_rng(n)
    targets = np.stack([np.stack([[so.scale_feature(x[r, s, e].astype(np.float64)) for e in range(E)] for s in range(S)])
                        for r in (11 + 97 * np.arange(Q)) % n])
    weights = 0.5 + rng.random((Q, S))
    return db, x, present, lost, targets, weights


@pytest.mark.parametrize("n", AWKWARD_N)
def test_batched_round_with_streams_that_lost_every_split(vqa, n):
    """Rows whose stream has no split present: avg NaN in that stream, n_e 0, score NaN, in neither list of any query and never the
    near arg-max -- also under bands that take every number (threshold below the minimum; lower = -inf).  Everywhere else the
    one-query round on the same handle and the oracle to <= 1e-12, and the lists == the NaN-aware numpy partition of the returned
    scores, exactly."""
    db, x, present, lost, targets, weights = _awkward_db(vqa, n, lose=True)
    Q = len(targets)
    first = db.query_round_batch(targets, weights, None)
    bands = np.empty((Q, 2))
    for q in range(Q):
        lo, hi = np.nanquantile(first[q].scores, [0.90, 0.97])
        bands[q] = (hi, lo)
    bands[2] = (np.nanmin(first[2].scores) - 1.0, np.nanmin(first[2].scores) - 2.0)           # every number matches
    bands[3] = (np.nanmax(first[3].scores) + 1.0, -np.inf)                                    # every number is near
    got = db.query_round_batch(targets, weights, bands)
    nan_rows = np.array(sorted(lost))
    numbers = np.setdiff1d(np.arange(n), nan_rows)
    for q, r in enumerate(got):
        assert same_bits(r.scores, first[q].scores) and same_bits(r.avg, first[q].avg)
        assert (r.n_e == present.sum(axis=2)).all() and (np.isnan(r.avg) == (r.n_e == 0)).all()
        for row, s in lost.items():
            assert np.isnan(r.avg[row, s]) and not np.isnan(r.avg[row, 1 - s]) and r.n_e[row, s] == 0 and np.isnan(r.scores[row])
        assert (np.flatnonzero(np.isnan(r.scores)) == nan_rows).all()
        assert not np.isin(nan_rows, r.match_rows).any() and not np.isin(nan_rows, r.near_rows).any() and r.near_argmax not in lost
        want = np_select(r.scores, bands[q, 0], bands[q, 1])
        assert (r.match_rows == want[0]).all() and (r.near_rows == want[1]).all() and r.near_argmax == want[2], q
        # the one-query round on the same handle, and the oracle
        one = db.query_round(targets[q], weights[q], tuple(bands[q]))
        assert (one.n_e == r.n_e).all() and (np.isnan(one.avg) == np.isnan(r.avg)).all() and (np.isnan(one.scores) == np.isnan(r.scores)).all()
        assert np.nanmax(np.abs(one.avg - r.avg)) <= TOL and np.nanmax(np.abs(one.scores - r.scores)) <= TOL, q
        _, o_avg, o_ne = so.dense_similarities(x, targets[q], present)
        assert (o_ne == r.n_e).all() and (np.isnan(o_avg) == np.isnan(r.avg)).all()
        assert np.nanmax(np.abs(o_avg - r.avg)) <= TOL and np.nanmax(np.abs(so.dense_scores(o_avg, weights[q]) - r.scores)) <= TOL, q
    assert (got[2].match_rows == numbers).all() and len(got[2].near_rows) == 0
    assert (got[3].near_rows == numbers).all() and len(got[3].match_rows) == 0 and got[3].near_argmax == int(np.nanargmax(got[3].scores))
    db.close()


@pytest.mark.parametrize("n", AWKWARD_N)
def test_batched_round_with_scores_exactly_on_the_band(vqa, n):
    """threshold == the score of row i and lower == the score of row j, bit for bit: i is a match (>=), j is near (lower <=); and a band
    (max, max): one match, nothing near."""
    db, _x, _present, _lost, targets, weights = _awkward_db(vqa, n, lose=False)
    Q = len(targets)
    first = db.query_round_batch(targets, weights, None)
    order = np.argsort(first[0].scores, kind="stable")
    i, j = int(order[(9 * n) // 10]), int(order[(6 * n) // 10])
    assert i != j and first[0].scores[j] < first[0].scores[i]
    bands = np.empty((Q, 2))
    for q in range(Q):
        lo, hi = np.quantile(first[q].scores, [0.90, 0.97])
        bands[q] = (hi, lo)
    bands[0] = (first[0].scores[i], first[0].scores[j])
    bands[1] = (first[1].scores.max(), first[1].scores.max())
    if n > 1024:                                              # a threshold below the minimum: all n rows match, longer than the prefix
        bands[2] = (first[2].scores.min() - 1.0, first[2].scores.min() - 2.0)
    got = db.query_round_batch(targets, weights, bands)
    # the planted values are the scores this call partitioned, bit for bit
    assert all(same_bits(r.scores, f.scores) for r, f in zip(got, first))
    assert same_bits(bands[0], got[0].scores[[i, j]]) and same_bits(bands[1], np.repeat(got[1].scores.max(), 2))
    assert i in got[0].match_rows and j in got[0].near_rows and j not in got[0].match_rows and i not in got[0].near_rows
    assert int((got[1].scores == got[1].scores.max()).sum()) == 1
    assert len(got[1].match_rows) == 1 and got[1].match_rows[0] == int(np.argmax(got[1].scores)) and len(got[1].near_rows) == 0
    assert got[1].near_argmax == -1
    if n > 1024:                                              # the fetched list is every row, and the other queries' lists stay their own
        assert len(got[2].match_rows) == n and (got[2].match_rows == np.arange(n)).all() and len(got[2].near_rows) == 0
    _check_partitions(got, bands)
    db.close()


@pytest.mark.parametrize("n", AWKWARD_N)
def test_every_flag_subset_of_a_batched_round_through_the_c_abi(vqa, n):
    """For every subset of {AVG, SCORES, SELECT}: the pieces asked for equal those of the flags-7 call bit for bit, the others keep the
    sentinel the block was filled with; vq_db_batch_round_fetch works only after SELECT (else VQ_E_STATE); vq_db_batch_round_times only
    after TIMED."""
    db, _x, _present, _lost, targets, weights = _awkward_db(vqa, n, lose=True)
    lib = vqa.load_library()
    Q, S, E, D = len(targets), db.S, db.E, db.D
    off = (C.c_int64 * 12)()
    vqa._lib.call("vq_db_batch_round_layout", db._h, Q, off)
    off = [int(v) for v in off]
    assert off == round_layout(Q, S, E, D, n=n)[0]
    p = C.c_void_p()
    vqa._lib.call("vq_host_alloc", C.byref(p), off[9])
    raw = np.ctypeslib.as_array((C.c_ubyte * off[9]).from_address(p.value))

    def view(piece, dtype, shape, src=None):
        count = int(np.prod(shape))
        return (raw if src is None else src)[off[piece]:off[piece] + count * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    scores0 = db.scan_batch(targets, weights)
    view(0, np.float64, (Q, S, E, D))[...] = targets
    view(1, np.float64, (Q, 8))[...] = 0.0
    view(1, np.float64, (Q, 8))[:, :S] = weights
    for q in range(Q):
        lo, hi = np.nanquantile(scores0[q], [0.5, 0.97])                                     # at n = 16 400 the near lists outgrow the prefix
        view(2, np.float64, (Q, 2))[q] = (hi, lo)
    bands = view(2, np.float64, (Q, 2)).copy()
    SENTINEL = 0xA5

    def run(flags):
        raw[off[3]:off[9]] = SENTINEL
        assert lib.vq_db_query_round_batch(db._h, Q, p, off[9], flags) == 0, lib.vq_last_error().decode()
        return raw.copy()

    def parts(block, bit):
        """what a piece holds (between and behind these the block is padding)"""
        if bit == 1:
            return [view(3, np.int32, (n, S), block), view(4, np.float64, (Q, n, S), block)]
        if bit == 2:
            return [view(5, np.float64, (Q, n), block)]
        res = view(6, np.int64, (Q, 4), block)
        out = [res]
        for q in range(Q):
            out.append(view(7, np.int64, (Q, off[10]), block)[q, :min(int(res[q, 0]), off[10])])
            out.append(view(8, np.int64, (Q, off[10]), block)[q, :min(int(res[q, 1]), off[10])])
        return out
    piece = {1: (off[3], off[5]), 2: (off[5], off[6]), 4: (off[6], off[9])}
    ms = (C.c_float * 3)()
    ref = run(7)
    assert same_bits(view(5, np.float64, (Q, n), ref), scores0)
    want = [np_select(scores0[q], bands[q, 0], bands[q, 1]) for q in range(Q)]
    assert [tuple(r[:3]) for r in view(6, np.int64, (Q, 4), ref)] == [(w[0].size, w[1].size, w[2]) for w in want]
    assert (max(w[1].size for w in want) > off[10]) == (n > 1024)
    for flags in range(8):
        out = run(flags)
        for bit, (a, b) in piece.items():
            if flags & bit:
                assert all(same_bits(g, r) for g, r in zip(parts(out, bit), parts(ref, bit))), (flags, bit)
            else:
                assert (out[a:b] == SENTINEL).all(), (flags, bit)
        for q in range(Q):
            m, k = np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int64)
            rc = lib.vq_db_batch_round_fetch(db._h, q, m.ctypes.data_as(C.c_void_p), n, k.ctypes.data_as(C.c_void_p), n)
            if flags & 4:
                assert rc == 0 and (m[:want[q][0].size] == want[q][0]).all() and (k[:want[q][1].size] == want[q][1]).all()
                assert (m[want[q][0].size:] == -7).all() and (k[want[q][1].size:] == -7).all()
            else:
                assert rc == -4 and (m == -7).all() and (k == -7).all()                       # VQ_E_STATE
        assert lib.vq_db_batch_round_times(db._h, ms) == -4                                  # not timed
    out = run(7 | 8)
    assert all(same_bits(g, r) for bit in piece for g, r in zip(parts(out, bit), parts(ref, bit)))
    assert lib.vq_db_batch_round_times(db._h, ms) == 0
    assert all(np.isfinite(v) and v >= 0.0 for v in ms), list(ms)
    run(2)
    assert lib.vq_db_batch_round_times(db._h, ms) == -4
    vqa._lib.call("vq_host_free", p)
    db.close()
