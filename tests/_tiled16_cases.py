"""Shared by tests/test_tiled16_gpu.py and tests/test_tiled16_host.py: the reference's goldens and cfg1_10k as a float16 database holds
them (rounded once to binary16), and the rule by which ranks of two scans that agree to 1e-12 are compared.

The recorded fp64 results of the goldens do not apply to a float16 database -- rounding the features moves every score -- so the tiled16
handle is compared with float16 ROWS holding the same halves.  Two handles whose scores agree to TOL can order two clips differently
only where the row-major scores of neighbours in rank lie within 2 TOL of each other; ranks are compared on the prefix before the first
such pair (``rank_prefix``), and that prefix must keep at least 99 % of the ranks (``MIN_KEPT``).  tests/test_tiled16_host.py checks that
bound for these inputs on the CPU, with the oracle on the rounded values."""
import numpy as np

import sim_oracle as so
from _helpers import golden_json, golden_npy, golden_target_array

TOL = 1e-12
GAP = 2 * TOL
MIN_KEPT = 0.99
GOLDENS = ["real_subset", "synth_small", "ragged"]
WEIGHTS = [1.0, 1.5]
CFG1_BAND = (0.8, 0.8 - 0.35 * 0.2)          # tests/test_sim_gpu.py::test_cfg1_10k_against_reference's select


def golden_case16(name):
    """(x [n,S,E,D] float16, clip ids, presence mask or None, target [S,E,D] float64) of one of the reference's goldens, rows in the
    golden's clip order, the features rounded to binary16."""
    g = golden_json(name + ".json")
    x = golden_npy(name + "_x.npy")
    ids = np.asarray(g.get("clip_ids") or g["clip_order"])
    present = np.array(g["present"], dtype=np.uint8) if "present" in g else None
    pos = {int(c): i for i, c in enumerate(ids)}
    rows = [pos[c] for c in g["clip_order"]]
    x16 = x[rows].astype(np.float16)
    assert np.isfinite(x16).all()
    return x16, np.asarray(g["clip_order"]), (present[rows] if present is not None else None), golden_target_array(g)


def cfg1_case16():
    """(x [10 000,2,3,1024] float16, target): cfg1_10k's features rounded to binary16, the query made from the rounded row 7."""
    x16 = so.cfg1_features(n=10000, e=3, seed=0).astype(np.float16)
    t = np.stack([[so.scale_feature(x16[7, s, e].astype(np.float64)) for e in range(3)] for s in range(2)])
    return x16, t


def rank_order(scores):
    """rows by descending score, ties by row, NaN last (stable)"""
    return np.argsort(-np.asarray(scores), kind="stable")


def rank_prefix(scores):
    """How many leading ranks of ``scores`` (the row-major scan's) are settled: every pair of neighbours in rank up to there is more than
    GAP apart.  All of them (the NaN tail included: its order is by row) when no pair is closer."""
    v = np.asarray(scores)[rank_order(scores)]
    v = v[~np.isnan(v)]
    close = np.flatnonzero(-np.diff(v) <= GAP)
    return int(close[0]) if close.size else int(np.asarray(scores).size)


def oracle_scores16(x16, t, present, w=WEIGHTS):
    _sims, avg, _ne = so.dense_similarities(x16.astype(np.float64), t, present)
    return so.dense_scores(avg, w)
