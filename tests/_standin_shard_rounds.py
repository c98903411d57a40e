"""Test stand-in: one rank's local database for the batched rounds of a ShardedFeatureDB -- TopOracleFeatureDB
(tests/test_batch_tickets_top_standin.py: the four calls of a batched round in numpy) with the rest of FeatureDB's surface that
ShardedFeatureDB asks of a local database: ``batch_round_supported``, ``query_round_batch`` with ``want_scores``, and
``batch_round_grid`` restated from the oracle.  Never imported by the product."""
import numpy as np

import sim_oracle as so
from test_batch_tickets_top_standin import TopOracleFeatureDB


class ShardRoundsFeatureDB(TopOracleFeatureDB):
    """``fail_on``: a value of the first weight of a call at which this rank's pass or re-weighting raises (a rank whose local step
    fails: the test sets it on one rank and then asks for that weight)."""

    fail_on = None

    def _maybe_fail(self, name, weights):
        if self.fail_on is not None and float(np.asarray(weights)[0][0]) == self.fail_on:
            raise RuntimeError("stand-in: this rank's %s fails" % name)

    def batch_round_supported(self):
        return self.D % 64 == 0 and self.S <= 8

    def query_round_batch(self, targets, weights, selects=None, want_avg=True, timed=False, want_scores=True):
        self._maybe_fail("query_round_batch", weights)
        out = super().query_round_batch(targets, weights, selects, True)     # the avg stays "on the device" (_kept) either way
        for r in out:
            if not want_avg:
                r.avg = r.n_e = None
            if not want_scores:
                r.scores = None
        return out

    def batch_round_grid(self, queries, rows, w_grids):
        self.log.append(("grid", list(queries)))
        out = []
        for q, r, wg in zip(queries, rows, w_grids):
            r = np.asarray(r, dtype=np.int64).reshape(-1)
            if r.size and (r.min() < 0 or r.max() >= self.n):
                raise ValueError("row outside [0,%d)" % self.n)
            out.append(np.stack([so.dense_scores(self._kept[q][0][r], w) for w in np.asarray(wg)]) if r.size else None)
        return out

    def batch_round_rescore(self, queries, weights, selects=None):
        self._maybe_fail("batch_round_rescore", weights)
        return super().batch_round_rescore(queries, weights, selects)
