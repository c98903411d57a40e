"""GPU: float16 storage of the feature database (VQ_F16) through the scans, the C ABI and the Python surface.

The parity statement is exact: binary16 -> binary64 widening loses nothing, so an fp16 database performs the fp64 arithmetic of the
other storage types on the ROUNDED values.  Tolerances (the project's, tests/test_sim_gpu.py):
  * dots / averaged similarities against the oracle fed the rounded values: |delta| <= 1e-12 (summation order only);
  * scores given the device's own averages, queries from a resident row, bootstrapped targets, the one-call round: bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sim_oracle as so
from _helpers import DEFAULT_WEIGHTS, STREAMS, golden_json, golden_npy, records_from_dense

pytestmark = pytest.mark.gpu
SIM_TOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
F16 = np.float16


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _rows16(rng, n, s, e, d, scales=(4.0, 1.0, 2.0)):
    x = rng.random((n, s, e, d))
    for si in range(s):
        x[:, si] *= scales[si]
    return x.astype(F16)


def _mask(rng, n, s, e, keep_one):
    p = (rng.random((n, s, e)) < 0.7).astype(np.uint8)
    if keep_one:
        p[..., 0] |= (p.sum(axis=2) == 0).astype(np.uint8)
    else:
        p[n // 2, s - 1, :] = 0                                            # a (clip, stream) without any split: no average
    return p


def _check_scan(db, x16, t, present, w):
    db.set_query(t)
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    o_sims, o_avg, o_ne = so.dense_similarities(x16.astype(np.float64), t, present)
    assert (n_e == o_ne).all()
    assert np.abs(sims - o_sims).max() <= SIM_TOL
    ok = ~np.isnan(o_avg)
    assert np.isnan(avg[~ok]).all()
    if ok.any():
        assert np.abs(avg[ok] - o_avg[ok]).max() <= SIM_TOL
    with np.errstate(invalid="ignore"):
        assert np.array_equal(db.scores(), so.dense_scores(avg, w), equal_nan=True)
    return avg, sims


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("s,e", [(1, 1), (2, 3), (2, 5)])
def test_fast_shapes_score_like_the_oracle_on_the_rounded_values(vqa, s, e, masked):
    d = 1024
    for n in (1, 5, 37, 2051):
        rng = np.random.default_rng(1000 * n + 10 * s + e)
        x16 = _rows16(rng, n, s, e, d)
        t = rng.standard_normal((s, e, d)) / d
        present = _mask(rng, n, s, e, keep_one=False) if masked else None
        w = [1.0, 1.5][:s]
        db = vqa.FeatureDB.from_arrays(x16, present=present, dtype=F16)
        assert db.dtype == F16 and (_bits(db.read_rows(np.arange(n))) == _bits(x16)).all()        # uploaded as is
        avg, sims = _check_scan(db, x16, t, present, w)
        db.scan(weights=w, keep_sims=True)
        avg2, _, sims2 = db.similarities(sims=True)
        assert np.array_equal(avg2, avg, equal_nan=True) and (sims2 == sims).all()                 # two scans of one handle: same bits
        db32 = vqa.FeatureDB.from_arrays(x16.astype(np.float32), present=present)                 # the same values in fp32 storage
        db32.set_query(t)
        db32.scan(keep_sims=True)
        avg32, _, sims32 = db32.similarities(sims=True)
        assert np.abs(sims32 - sims).max() <= SIM_TOL
        ok = ~np.isnan(avg)
        assert (np.isnan(avg32) == ~ok).all() and (not ok.any() or np.abs(avg32[ok] - avg[ok]).max() <= SIM_TOL)
        db32.close()
        db.close()


def test_every_k_position_meets_its_query_value(vqa):
    """One-hot rows: row c, vector v has its single non-zero at k = (7 c + 131 v) mod 1024 and the query holds a distinct value per k.
    Every dot has one term and an exact product: any mismatch between the 8-halves-per-lane load order and the LDS image of the query
    shows as an unequal similarity, at every one of the 1 024 positions."""
    n, s, e, d = 2048, 2, 3, 1024
    x = np.zeros((n, s, e, d), dtype=F16)
    c = np.arange(n)
    for v in range(s * e):
        x[c, v // e, v % e, (7 * c + 131 * v) % d] = 1.0 + 0.25 * (c % 7)
    t = ((1.0 + np.arange(s * e * d)) * 2.0 ** -16).reshape(s, e, d)
    db = vqa.FeatureDB.from_arrays(x, dtype=F16)
    db.set_query(t)
    db.scan(keep_sims=True)
    sims = db.similarities(sims=True)[2]
    o_sims = so.dense_similarities(x.astype(np.float64), t)[0]
    assert (sims == o_sims).all()
    # the 16-query pass reads the query rows in its own element order: same rows, sixteen scaled copies of the query
    targets = np.stack([t * 2.0 ** -q for q in range(16)])
    weights = np.ones((16, s))
    got = db.scan_batch(targets, weights)
    for q in (0, 5, 15):
        avg = so.dense_similarities(x.astype(np.float64), targets[q])[1]
        assert np.abs(got[q] - so.dense_scores(avg, weights[q])).max() <= SIM_TOL
    db.close()


@pytest.mark.parametrize("lean", [0, 1])
def test_waves_that_loop_in_both_instantiations(gpu, lean):
    """tests/_f16_scan_child.py: VQ_SCAN_LEAN is read once per process, so each instantiation of the fast kernel gets a fresh one --
    one-hot rows exactly, then 40 003 clips (every wave walks 13 or 14, the last round is ragged) sampled against the oracle."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_f16_scan_child.py"), str(lean)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", [64, 260])
def test_generic_kernel(vqa, d, masked):
    n, s, e = 50, 3, 2
    rng = np.random.default_rng(d)
    x16 = _rows16(rng, n, s, e, d)
    t = rng.standard_normal((s, e, d)) / d
    present = _mask(rng, n, s, e, keep_one=False) if masked else None
    db = vqa.FeatureDB.from_arrays(x16, present=present, dtype=F16)
    _check_scan(db, x16, t, present, [1.0, 1.5, 0.5])
    assert (_bits(db.read_rows([0, 7, n - 1])) == _bits(x16[[0, 7, n - 1]])).all()                # rows of 8-byte units (D = 260)
    db.close()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("d", [256, 1024])
def test_sixteen_query_pass(vqa, d, masked):
    s, e = 2, 3
    for n in (1, 37, 1000):
        rng = np.random.default_rng(n + d)
        x16 = _rows16(rng, n, s, e, d)
        present = _mask(rng, n, s, e, keep_one=True) if masked else None
        db = vqa.FeatureDB.from_arrays(x16, present=present, dtype=F16)
        t1 = rng.standard_normal((s, e, d)) / d
        db.set_query(t1)
        db.scan(weights=[1.0, 1.5])
        avg1, sc1 = db.similarities()[0], db.scores()
        x64 = x16.astype(np.float64)
        for q in (1, 7, 16):
            targets = rng.standard_normal((q, s, e, d)) / d
            weights = 0.5 + rng.random((q, s))
            got = db.scan_batch(targets, weights)
            assert got.shape == (q, n)
            for k in range(q):
                avg = so.dense_similarities(x64, targets[k], present)[1]
                assert np.abs(got[k] - so.dense_scores(avg, weights[k])).max() <= SIM_TOL, (n, q, k)
            assert (db.scan_batch(targets, weights) == got).all()
        assert (db.similarities()[0] == avg1).all() and (db.scores() == sc1).all()                # the one-query state is untouched
        db.close()


def test_generated_rows_are_the_host_generator_rounded_to_nearest_even(vqa):
    n, s, e, d, scales = 300, 2, 3, 1024, (4.0, 1e-4)
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=41, scales=scales, row0=77, dtype=F16)
    x16 = so.synth_features(41, 77, n, s, e, d, scales).astype(F16)
    tiny = x16[:, 1]
    assert ((tiny != 0) & (np.abs(tiny) < 2.0 ** -14)).mean() > 0.3                             # stream 1 is mostly subnormal halves
    assert (_bits(db.read_rows(np.arange(n))) == _bits(x16)).all()
    rng = np.random.default_rng(41)
    _check_scan(db, x16, rng.standard_normal((s, e, d)) / d, None, [1.0, 1.5])                     # subnormals survive the widening
    t = np.zeros((s, e, d))
    t[1] = rng.standard_normal((e, d)) * 1e3                                                       # the subnormal stream alone, amplified
    db.set_query(t)
    db.scan(keep_sims=True)
    sims = db.similarities(sims=True)[2]
    o_sims = so.dense_similarities(x16.astype(np.float64), t)[0]
    assert np.abs(o_sims[:, 1]).max() > 1e-3 and np.abs(sims - o_sims).max() <= SIM_TOL
    db.close()


def test_upload_read_rows_and_adopted_memory_keep_bits(vqa):
    import torch
    n, s, e, d = 50, 2, 3, 1024
    rng = np.random.default_rng(3)
    x16 = _rows16(rng, n, s, e, d)
    db = vqa.FeatureDB(n, s, e, d, dtype=F16)
    db.upload(0, np.zeros((n, s, e, d), dtype=F16))
    db.upload(10, x16[10:30])
    rows = [29, 10, 17, 9, 30]
    got = db.read_rows(rows)
    assert got.dtype == F16 and (_bits(got[:3]) == _bits(x16[[29, 10, 17]])).all() and (_bits(got[3:]) == 0).all()
    db.upload(0, x16.astype(np.float64))                                     # host conversion: numpy's astype
    assert (_bits(db.read_rows(np.arange(n))) == _bits(x16)).all()
    t = rng.standard_normal((s, e, d)) / d
    db.set_query(t)
    db.scan(weights=[1.0, 1.5], keep_sims=True)
    want = db.similarities(sims=True)
    dev = torch.from_numpy(x16).cuda()
    assert dev.dtype == torch.float16
    ad = vqa.FeatureDB(n, s, e, d, dtype=F16)
    ad.adopt_device(dev.data_ptr(), keepalive=dev)
    ad.set_query(t)
    ad.scan(weights=[1.0, 1.5], keep_sims=True)
    got = ad.similarities(sims=True)
    assert all((a == b).all() for a, b in zip(got, want)) and (ad.scores() == db.scores()).all()
    ad.close()
    db.close()


def test_resident_row_queries_and_bootstrapped_targets_equal_fp32_storage_bit_for_bit(vqa):
    n, s, e, d = 120, 2, 3, 1024
    x16 = _rows16(np.random.default_rng(9), n, s, e, d)
    db = vqa.FeatureDB.from_arrays(x16, dtype=F16)
    db32 = vqa.FeatureDB.from_arrays(x16.astype(np.float32))
    t16, t32 = db.set_query_from_row(7), db32.set_query_from_row(7)
    assert (t16 == t32).all()
    r = x16[7].astype(np.float64)
    assert np.abs(t16 - r / (r * r).sum(axis=-1, keepdims=True)).max() <= 1e-15
    db.scan(weights=[1.0, 1.5])
    assert db.scores().argmax() == 7
    for valid, invalid, mu in (([7, 8, 9, 10], [], 0.0), ([7, 8, 9, 10], [100, 101, 102], 0.3)):
        b16 = db.bootstrap_target(valid, invalid, mu=mu, set_query=False)
        b32 = db32.bootstrap_target(valid, invalid, mu=mu, set_query=False)
        assert np.isfinite(b16).all() and (b16 == b32).all()
    db32.close()
    db.close()


def test_the_one_call_round_equals_the_separate_calls(vqa):
    n, s, e, d = 999, 2, 3, 1024
    rng = np.random.default_rng(12)
    x16 = _rows16(rng, n, s, e, d)
    p = _mask(rng, n, s, e, keep_one=True)
    db = vqa.FeatureDB.from_arrays(x16, present=p, dtype=F16)
    t = x16[7].astype(np.float64)
    t = t / (t * t).sum(axis=-1, keepdims=True)
    for w, th, lower in ((np.array([1.0, 1.5]), 0.8, 0.73), (np.array([1.0, 0.5]), 0.25, 0.1)):
        db.set_query(t)
        db.scan()
        avg, n_e = db.similarities()
        db.rescore(w)
        scores = db.scores()
        m, q, am = db.select(th, lower)
        r = db.query_round(t, weights=w, select=(th, lower))
        assert (r.avg == avg).all() and (r.n_e == n_e).all() and (r.scores == scores).all()
        assert (r.match_rows == m).all() and (r.near_rows == q).all() and r.near_argmax == am
    db.close()


def test_refusals(vqa):
    n, s, e, d = 200, 2, 2, 1024
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=3, scales=(2.0, 1.0), dtype=F16)
    with pytest.raises(vqa.VqError) as ei:
        db.set_layout("tiled")
    assert ei.value.code == -5 and db.layout == "rows"
    x16 = so.synth_features(3, 0, n, s, e, d, (2.0, 1.0)).astype(F16)
    _check_scan(db, x16, np.random.default_rng(0).standard_normal((s, e, d)) / d, None, [1.0, 1.5])   # the handle keeps working
    db.close()
    big = np.ones((2, 1, 1, 8))
    big[1, 0, 0, 5] = 70000.0
    with pytest.raises(ValueError, match=r"\(1, 0, 0, 5\)"):
        vqa.FeatureDB.from_arrays(big, dtype=F16)
    edge = vqa.FeatureDB.from_arrays(np.full((1, 1, 1, 8), 65519.0), dtype=F16)                   # rounds to 65504, the largest half
    assert (edge.read_rows([0]) == F16(65504.0)).all()
    edge.close()
    widened = vqa.FeatureDB.from_arrays(np.ones((2, 1, 1, 8), dtype=F16))                          # no dtype: float16 input is widened
    assert widened.dtype == np.float32
    widened.close()
    with pytest.raises(TypeError):
        vqa.FeatureDB(4, 1, 1, 8, dtype=np.int8)


def test_ticket_round_on_a_float16_database(vqa):
    import random
    g = golden_json("synth_small.json")
    x = golden_npy("synth_small_x.npy")
    ids = np.asarray(g["clip_order"])
    recs = records_from_dense(x, ids, [1, 2, 3])
    tk = vqa.Ticket({"query_id": 1, "video_id": 1, "ref_clip": 0, "ref_clip_id": g["ref_clip_id"], "search_set": 1,
                     "number_of_matches_to_review": 20, "dynamic_target_adjustment": False, "user_matches": g.get("user_matches", {})},
                    records=recs)
    hp = vqa.Hyperparameter(DEFAULT_WEIGHTS, 0.8, 0.0, 0.35, 0.0, STREAMS, "global_pool", 1, 0.7, "bagging", 3)
    tk.target = vqa.TargetClip(tk, hp)
    tk.target.get_target_features()
    tf = tk.target.target_features
    db64 = vqa.FeatureDB.from_records(recs, tf, STREAMS, "global_pool", dtype=np.float64)
    db16 = vqa.FeatureDB.from_records(recs, tf, STREAMS, "global_pool", dtype=F16)
    assert (db16.clip_ids == db64.clip_ids).all()
    rows = np.arange(db64.n)
    x16 = db16.read_rows(rows)
    assert x16.dtype == F16 and (_bits(x16) == _bits(db64.read_rows(rows).astype(F16))).all()
    names, splits = db16.stream_names, db16.slot_splits
    db64.close()
    db16.close()
    tk.feature_db_dtype = F16
    tk.compute_similarities(hp)
    assert tk.feature_db.dtype == F16
    t = np.array([[tf[st][sp] for sp in splits[si]] for si, st in enumerate(names)], dtype=np.float64)
    _, o_avg, o_ne = so.dense_similarities(x16.astype(np.float64), t)
    for row, c in enumerate(tk.feature_db.clip_ids.tolist()):
        for si, st in enumerate(names):
            assert abs(tk.similarities[c][st][0] - o_avg[row, si]) <= SIM_TOL and tk.similarities[c][st][1] == o_ne[row, si]
    tk.compute_scores(DEFAULT_WEIGHTS)
    assert len(tk.scores) == len(ids) and all(np.isfinite(v) for v in tk.scores.values())
    random.seed(a=1)
    tk.select_clips_to_review(0.8, 20, 0.35)
    assert len(tk.matches) >= 1
    tk.feature_db.close()


def test_one_rccl_rank_equals_the_plain_database(gpu):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_f16_sharded.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
