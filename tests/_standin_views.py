"""Test stand-in: tests/_standin_db.py's numpy database plus search sets (row views), with the surface FeatureDB gives them --
define_search_set / define_search_rows / use_search_set / drop_search_set / has_search_set -- restated in numpy: while a set is in use
the stand-in scans only its rows, and every result array and row argument is a position in the set."""
import numpy as np
import sim_oracle as so
from _standin_db import OracleFeatureDB

from video_query_algorithms_amd.feature_db import SearchSetView, search_set_rows, whole_view


class ViewOracleFeatureDB(OracleFeatureDB):
    def __init__(self, feats, present=None, stream_names=None, slot_splits=None, fail_on_scan=False, clip_ids=None):
        super().__init__(feats, present, stream_names, slot_splits, fail_on_scan)
        self.clip_ids = np.arange(1, self.n + 1, dtype=np.int64) if clip_ids is None else np.asarray(clip_ids, dtype=np.int64)
        self._index = {int(c): i for i, c in enumerate(self.clip_ids.tolist())}
        self._sets, self._in_use, self._whole = {}, None, None
        self.use_calls = 0                                   # how often the set in use CHANGED (what costs a library call)

    # index of the whole database
    def row_of(self, clip_id):
        return self._index[int(clip_id)]

    def has_clip(self, clip_id):
        try:
            return int(clip_id) in self._index
        except (TypeError, ValueError):
            return False

    # search sets
    def define_search_set(self, set_id, clip_ids):
        return self.define_search_rows(set_id, search_set_rows(self, clip_ids))

    def define_search_rows(self, set_id, rows):
        r = np.asarray(rows, dtype=np.int64).reshape(-1)
        if set_id is None or set_id in self._sets:
            raise ValueError("bad or repeated search set id %r" % (set_id,))
        if r.size and (r.min() < 0 or r.max() >= self.n or (np.diff(r) <= 0).any()):
            raise ValueError("rows must be strictly ascending in [0,%d)" % self.n)
        self._sets[set_id] = SearchSetView(set_id, self.clip_ids[r], r)
        return self._sets[set_id]

    def has_search_set(self, set_id):
        try:
            return set_id is not None and set_id in self._sets
        except TypeError:
            return False

    def use_search_set(self, set_id):
        if set_id is None:
            if self._whole is None:
                self._whole = whole_view(self)
            view = self._whole
        else:
            view = self._sets[set_id]
        if set_id != self._in_use:
            self._in_use = set_id
            self.use_calls += 1
            self._avg = self._ne = self._scores = self._sims = None
        return view

    def drop_search_set(self, set_id):
        if set_id == self._in_use:
            raise RuntimeError("search set %r is in use" % (set_id,))
        del self._sets[set_id]

    def _rows(self):
        return None if self._in_use is None else self._sets[self._in_use].rows

    # the scan over the set in use
    def _effective(self):
        base = super()._effective()
        return base if self._rows() is None else base[self._rows()]

    def scan(self, weights=None, keep_sims=False):
        if self.fail_on_scan:
            raise RuntimeError("stand-in: this rank's scan fails")
        x = self.x if self._rows() is None else self.x[self._rows()]
        self._sims, self._avg, self._ne = so.dense_similarities(x, self._t, self._effective())
        self._scores = None if weights is None else so.dense_scores(self._avg, weights)

    def scan_batch(self, targets, weights, want=True):
        if self._rows() is not None:
            raise RuntimeError("the batched scan runs over the whole database")
        return super().scan_batch(targets, weights, want)

    def topk(self, k):
        v = self._scores                                     # as the device: descending, ties by ascending position, NaNs excluded
        idx = np.flatnonzero(~np.isnan(v))
        order = idx[np.lexsort((idx, -v[idx]))][:k]
        return order.astype(np.int64), v[order]
