"""Test infrastructure (GPU box): one table of tests/_dot_cases.py through one path of csrc/vq_sim.hip or csrc/vq_sim_batch.hip -- shared by
tests/test_dot_hard_gpu.py (this process) and tests/_dot_hard_child.py (one process per forced scan_kernel instantiation).

Every function returns a ``Visit``: the worst |err| / bound per family and how many scans ran, so that a test can assert what it
covered."""
import numpy as np

import sim_oracle as so
import _dot_cases as dc
from _search_set_cases import same_bits, same_values


SCAN_SHAPES = [(1, 1), (2, 3), (2, 5)]                         # scan_kernel at D = 1024 (tests/_dot_hard_child.py)


def cell_line(s, e, group):
    """What a child prints per (shape, group) and the parent looks for."""
    return "cell %d x %d %s:" % (s, e, group)


class Visit:
    def __init__(self):
        self.worst, self.scans, self.finite, self.classes = {}, 0, 0, 0

    def add(self, checked):
        worst, n_fin, n_cls = checked
        for f, v in worst.items():
            self.worst[f] = max(self.worst.get(f, 0.0), v)
        self.scans += 1
        self.finite += n_fin
        self.classes += n_cls

    def merge(self, other):
        for f, v in other.worst.items():
            self.worst[f] = max(self.worst.get(f, 0.0), v)
        self.scans += other.scans
        self.finite += other.finite
        self.classes += other.classes
        return self

    def line(self):
        return "%s (%d scans, %d finite values, %d classes)" % (dc.ratio_line(self.worst), self.scans, self.finite, self.classes)


def _scan(db, w):
    db.scan(weights=w, keep_sims=True)
    avg, n_e, sims = db.similarities(sims=True)
    return avg, n_e, sims, db.scores()


def masked_facts(tb, exp, avg, n_e, rows=None):
    """under the table's mask: a non-finite row's means are finite when another split is there, a (clip, stream) without a split is NaN"""
    rows = np.arange(tb.n) if rows is None else rows
    assert (np.isnan(avg) == (n_e == 0)).all() and (n_e == 0).sum() >= 1
    at = np.flatnonzero(np.isin(rows, tb.nonfinite_rows))
    assert at.size == tb.nonfinite_rows.size
    assert np.isfinite(avg[at]).all() if tb.E > 1 else np.isnan(avg[at]).all()


def one_query_path(vqa, tb, layout="rows", view_rows=None):
    """The table through FeatureDB.scan, plain and under its presence mask, each as a full scan (twice: the same bits) and under a
    row view (bit for bit the full scan's rows): sims and avg against bound and class, n_e exact, scores bit for bit from the device's
    avg.  ``layout`` "tiled": the block must read back bit for bit after tiling and after going back to rows, compared as integers."""
    w = dc.WEIGHTS[:tb.S]
    view_rows = tb.view_rows() if view_rows is None else view_rows
    visit = Visit()
    db = vqa.FeatureDB.from_arrays(tb.x, dtype=tb.dtype)
    assert db.dtype == tb.dtype
    if layout == "tiled":
        as_int = tb.x.view(np.uint32)
        every = np.arange(tb.n)
        assert (db.read_rows(every).view(np.uint32) == as_int).all()
        db.set_layout("tiled")
        assert db.layout == "tiled" and (db.read_rows(every).view(np.uint32) == as_int).all(), "tiled"
        db.set_layout("rows")
        assert db.layout == "rows" and (db.read_rows(every).view(np.uint32) == as_int).all(), "back to rows"
        db.set_layout("tiled")
    db.set_query(tb.t)
    for masked in (False, True):
        db.set_present(tb.mask() if masked else None)
        exp = tb.expected(masked)
        full = _scan(db, w)
        avg, n_e, sims, sc = full
        visit.add(dc.check_against(exp, tb.family, avg, n_e, sims))
        assert same_values(sc, so.dense_scores(avg, w)), "scores"
        assert all(same_bits(a, b) for a, b in zip(_scan(db, w), full)), "second scan"
        if masked:
            masked_facts(tb, exp, avg, n_e)
        db.define_search_rows("v", view_rows)
        db.use_search_set("v")
        got = _scan(db, w)
        assert got[0].shape == (view_rows.size, tb.S) and got[2].shape == (view_rows.size, tb.S, tb.E)
        assert all(same_bits(a, b[view_rows]) for a, b in zip(got, full)), "view"
        visit.add(dc.check_against(exp, tb.family, got[0], got[1], got[2], rows=view_rows))
        db.use_search_set(None)
        db.drop_search_set("v")
    db.close()
    return visit


def batched_path(vqa, tb, Qs=(1, 7, 16), layout="rows"):
    """The table through query_round_batch (want_avg), scan_batch and query_round_batch_sets, for every Q, plain and masked.  Query q
    is dc.query_variant(tb, q): the ``pos_inf`` row is +inf, -inf and NaN under neighbouring queries of one pass."""
    visit = Visit()
    db = vqa.FeatureDB.from_arrays(tb.x, dtype=tb.dtype)
    assert db.batch_round_supported()
    if layout == "tiled":
        db.set_layout("tiled")
    rows_v = tb.tile_view_rows() if layout == "tiled" else tb.view_rows()
    db.define_search_rows("v", rows_v)
    every = np.arange(tb.n)
    for masked in (False, True):
        db.set_present(tb.mask() if masked else None)
        for Q in Qs:
            targets = np.stack([dc.query_variant(tb, q) for q in range(Q)])
            weights = np.array([[wv * (1.0 + 0.125 * (q % 5)) for wv in dc.WEIGHTS[:tb.S]] for q in range(Q)])
            got = [(np.array(r.avg), np.array(r.n_e), np.array(r.scores)) for r in db.query_round_batch(targets, weights, None, want_avg=True)]
            assert len(got) == Q
            for q, (avg, n_e, sc) in enumerate(got):
                exp = tb.expected(masked, q)
                visit.add(dc.check_against(exp, tb.family, avg, n_e))
                assert same_values(sc, so.dense_scores(avg, weights[q])), ("scores", Q, q)
                if masked:
                    masked_facts(tb, exp, avg, n_e)
            assert same_bits(db.scan_batch(targets, weights), np.stack([g[2] for g in got])), "scan_batch"
            again = db.query_round_batch(targets, weights, None, want_avg=True)
            assert all(same_bits(np.array(r.avg), g[0]) and same_bits(np.array(r.scores), g[2]) for r, g in zip(again, got)), "second round"
            set_ids = ["v" if q % 2 else None for q in range(Q)]
            sets = db.query_round_batch_sets(targets, weights, set_ids, None, want_avg=True)
            for q, r in enumerate(sets):
                rows = rows_v if set_ids[q] else every
                assert same_bits(np.array(r.avg), got[q][0][rows]) and same_bits(np.array(r.n_e), got[q][1][rows]) and same_bits(np.array(r.scores), got[q][2][rows]), ("sets", Q, q)
                visit.add(dc.check_against(tb.expected(masked, q), tb.family, np.array(r.avg), np.array(r.n_e), rows=rows))
    db.drop_search_set("v")
    db.close()
    return visit
