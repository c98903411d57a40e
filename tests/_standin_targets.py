"""Test stand-in: the numpy database of tests/test_batch_tickets_standin.py plus target bootstrapping on resident rows, restated from
the oracle -- ``bootstrap_target`` (one draw: oracle.kernel_order_target per slot, what csrc/vq_boot.hip computes) and, one class
further, ``batch_targets`` (every draw of several queries: the same per draw, numpy's sequential mean over the draws, the blend of
target_clip.py:75-82).  ``log`` records ("boot", rows) per one-draw call and ("targets", pool sizes) per batched call.  Never
imported by the product."""
import numpy as np

import bootstrap_oracle as bo
from test_batch_tickets_standin import RoundOracleFeatureDB

from video_query_algorithms_amd import VqError

_SOLVED = {}          # (id of the feature block, rows, n_valid, mu) -> [S][E][D]: one solve per distinct draw and process


class BootOracleFeatureDB(RoundOracleFeatureDB):
    def _draw_target(self, valid_rows, invalid_rows, mu):
        v, iv = [int(r) for r in valid_rows], [int(r) for r in invalid_rows]
        key = (id(self.x), tuple(v), tuple(iv), float(mu))
        if key not in _SOLVED:
            out = np.empty((self.S, self.E, self.D))
            for s in range(self.S):
                for e in range(self.E):
                    X = self.x[v, s, e].astype(np.float64)
                    Y = self.x[iv, s, e].astype(np.float64) if iv else None
                    try:
                        out[s, e] = bo.kernel_order_target(X, Y, float(mu))[0]
                    except bo.SingularSystem:
                        out = s * self.E + e
                        break
                if isinstance(out, int):
                    break
            _SOLVED[key] = out
        return _SOLVED[key]

    def bootstrap_target(self, valid_rows, invalid_rows=(), mu=0.0, set_query=True):
        self.log.append(("boot", list(valid_rows) + list(invalid_rows)))
        t = self._draw_target(valid_rows, invalid_rows, mu)
        if isinstance(t, int):
            raise VqError(-1, "problem %d: singular system (linearly dependent validated clips) -- numpy.linalg.inv raises here too" % t)
        if set_query:
            self.set_query(t)
        return t.copy()


class TargetsOracleFeatureDB(BootOracleFeatureDB):
    def batch_targets(self, pools, draws, mus, previous=None, keeps=None):
        if not 1 <= len(pools) <= 16:
            raise ValueError("1 to 16 queries per call")
        self.log.append(("targets", [len(v) + len(iv) for v, iv in pools]))
        out = []
        for q, ((valid, invalid), picks, mu) in enumerate(zip(pools, draws, mus)):
            acc = None
            for b, (pv, pi) in enumerate(picks):
                w = self._draw_target([valid[i] for i in pv], [invalid[i] for i in pi], mu)
                if isinstance(w, int):
                    raise VqError(-1, "query %d, draw %d: problem %d: singular system (linearly dependent validated clips) -- numpy.linalg.inv "
                                  "raises here too" % (q, b, w))
                acc = w if acc is None else acc + w
            t = acc if len(picks) == 1 else acc / len(picks)
            if previous is not None and previous[q] is not None:
                t = np.multiply(keeps[q], t) + np.multiply((1 - keeps[q]), previous[q])
            out.append(t)
        return out
