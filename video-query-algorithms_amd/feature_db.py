"""Resident feature database on one MI355X: the host-side handle over ``vq_db_*``.

The reference keeps no database object: every query re-downloads all features of the search set
as JSON and regroups them into ``{stream: {split: {clip: list}}}``
(``Ticket._get_candidate_features``, src/models/ticket.py:358-382).  ``FeatureDB`` holds the same
information as one ``[N][S][E][D]`` block in HBM plus the clip-id index and the order in which the
reference would have met the clips (which fixes the iteration order of ``ticket.similarities`` and
with it what ``random.sample`` draws in ``select_clips_to_review``).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Iterable, Mapping, Sequence

import numpy as np

from . import _lib
from ._lib import VQ_F16, VQ_F32, VQ_F64, call

_VQ_DTYPE = {np.dtype(np.float16): VQ_F16, np.dtype(np.float32): VQ_F32, np.dtype(np.float64): VQ_F64}


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class _RoundBlock:
    """One page-locked host block of vq_db_query_round (include/vq_amd.h), exposed to numpy.  The arrays a round hands out are views
    of it; when the last of them is gone the block goes back to its database's pool (or is freed if the database is)."""

    def __init__(self, ptr: int, nbytes: int, pool: dict):
        self.ptr, self.nbytes, self._pool = ptr, nbytes, pool
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def bytes(self) -> np.ndarray:
        return np.asarray(self)                               # its .base is self: views of it keep the block out of the pool

    def __del__(self):
        pool = self._pool
        if not pool["closed"] and len(pool["free"]) < 4:
            pool["free"].append((self.ptr, self.nbytes))      # reborn as a fresh _RoundBlock by the next round
        else:
            try:
                _lib.load().vq_host_free(C.c_void_p(self.ptr))
            except Exception:
                pass


class RoundResult:
    """What one call of :meth:`FeatureDB.query_round` brought back (numpy views of one page-locked block)."""
    __slots__ = ("avg", "n_e", "scores", "match_rows", "near_rows", "near_argmax")


class UpdateResult(RoundResult):
    """What :meth:`FeatureDB.batch_round_update` brought back for one query: the fields of the rescore's :class:`RoundResult` and the
    pick -- ``w`` (the fitted grid weight), ``threshold``, ``lowest`` (the lowest-scoring confirmed match of a finalize member, else
    1.0), ``band`` = (threshold, lower), ``iw`` / ``it`` (the cell), ``on_rim``, ``fell_back``, and ``surface`` [G,T] when asked."""
    __slots__ = ("w", "threshold", "lowest", "band", "iw", "it", "on_rim", "fell_back", "surface")


class SearchSetView:
    """What a ticket sees of a database for one round: the clips of its search set, in database order.  Immutable -- a ticket binds
    to this object, not to the (shared, mutable) state of the handle.  ``clip_ids`` [M] and ``rows`` [M] (the database rows, strictly
    ascending); a clip's POSITION in the view is what the database's result arrays and row arguments are indexed by while the
    view is in use.  The trivial view (``set_id`` None) is the whole database: positions are rows."""
    __slots__ = ("set_id", "clip_ids", "rows", "n", "token", "_pos", "_whole")

    def __init__(self, set_id, clip_ids: np.ndarray, rows: np.ndarray, token: int = -1, whole=None):
        ids, r = np.asarray(clip_ids, dtype=np.int64), np.asarray(rows, dtype=np.int64)
        if whole is None:                                     # the trivial view shares the database's own arrays and index
            ids, r = ids.copy(), r.copy()
            ids.setflags(write=False)
            r.setflags(write=False)
        for name, value in (("set_id", set_id), ("clip_ids", ids), ("rows", r), ("n", int(ids.shape[0])), ("token", int(token)),
                            ("_pos", None), ("_whole", whole)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a search-set view is immutable")

    def row_of(self, clip_id) -> int:
        """The clip's position in the view; ``KeyError`` for a clip outside the search set."""
        if self._whole is not None:
            return self._whole.row_of(clip_id)
        if self._pos is None:
            object.__setattr__(self, "_pos", {int(c): i for i, c in enumerate(self.clip_ids.tolist())})      # a cache, not state
        return self._pos[int(clip_id)]

    def has_clip(self, clip_id) -> bool:
        try:
            self.row_of(clip_id)
            return True
        except (KeyError, TypeError, ValueError):
            return False


def whole_view(db) -> SearchSetView:
    """The trivial view of a database object (FeatureDB, ShardedFeatureDB, or a look-alike with ``clip_ids`` and ``row_of``)."""
    n = len(db.clip_ids)
    return SearchSetView(None, db.clip_ids, np.arange(n, dtype=np.int64), whole=db)


def search_set_rows(db, clip_ids) -> np.ndarray:
    """Clip ids -> the strictly ascending database rows of a search set (duplicates collapse; an unknown id is a KeyError)."""
    return np.unique(np.fromiter((db.row_of(c) for c in clip_ids), dtype=np.int64))


class FeatureDB:
    """N clips x S streams x E ensemble slots x D floats, resident on ``device``.  ``dtype`` is how the block is STORED: float32, float64
    or (opt-in) float16 -- half the bytes per query and per clip; values are rounded once on the way in and every result is what the
    fp64 arithmetic gives on the rounded values."""

    def __init__(self, n: int, n_streams: int, n_splits: int, dim: int = 1024, dtype=np.float32, device: int = 0,
                 clip_ids: Sequence[int] | None = None):
        self.n, self.S, self.E, self.D = int(n), int(n_streams), int(n_splits), int(dim)
        self.dtype = np.dtype(dtype)
        if self.dtype not in _VQ_DTYPE:
            raise TypeError("FeatureDB dtype must be float32, float64 or float16")
        self.device = int(device)
        self._h = C.c_void_p()
        call("vq_db_create", self.n, self.S, self.E, self.D, _VQ_DTYPE[self.dtype], self.device, C.byref(self._h))
        self.clip_ids = (np.arange(1, self.n + 1, dtype=np.int64) if clip_ids is None
                         else np.asarray(clip_ids, dtype=np.int64).copy())
        if self.clip_ids.shape != (self.n,):
            raise ValueError("clip_ids must have shape (%d,)" % self.n)
        self._row_of = None
        self.present = None
        self._keepalive = None
        # One resident database may serve several tickets.  The query, the averaged similarities and the scores
        # are state of the HANDLE, and a round is several calls (ticket.py:96-170): ``lock`` (re-entrant) makes a group of calls
        # atomic, ``sims_owner`` / ``scores_owner`` say whose similarities / scores the device holds right now, so a ticket that finds
        # another ticket's there puts its own back (TicketScoring._own_similarities) instead of scoring with a stranger's query.
        self.lock = threading.RLock()
        self.sims_owner = None
        self.scores_owner = None
        # search sets (define_search_set): id -> view; the one the handle runs over now (None: the whole database) and how many
        # clips the result arrays then cover
        self._sets = {}
        self._set_in_use = None
        self._whole = None
        self._na = self.n
        # the layout of a one-query round's block and the pool of its page-locked blocks: made here, so that the first rounds of two
        # threads share one pool
        off = (C.c_int64 * 10)()
        call("vq_db_round_layout", self._h, off)
        self._round_off = [int(v) for v in off]
        self._round_pool = {"free": [], "closed": False}

    # ------------------------------------------------------------------ search sets
    def define_search_set(self, set_id, clip_ids):
        """Make the clips ``clip_ids`` (any order; duplicates collapse; an id the database does not hold is a ``KeyError``) a search
        set of this database: its ascending rows go to the device once (vq_db_rows_define) and stay there until
        :meth:`drop_search_set`.  Returns the view object."""
        return self.define_search_rows(set_id, search_set_rows(self, clip_ids))

    def define_search_rows(self, set_id, rows):
        """The same from database rows (strictly ascending)."""
        if set_id is None:
            raise ValueError("None names the whole database")
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        with self.lock:
            if set_id in self._sets:
                raise ValueError("search set %r is already defined (drop_search_set first)" % (set_id,))
            vid = C.c_int32(-1)
            call("vq_db_rows_define", self._h, _np_ptr(r) if r.size else None, int(r.size), C.byref(vid))
            view = SearchSetView(set_id, self.clip_ids[r], r, token=vid.value)
            self._sets[set_id] = view
            return view

    def has_search_set(self, set_id) -> bool:
        try:
            return set_id is not None and set_id in self._sets
        except TypeError:                                     # an unhashable id names no set
            return False

    def use_search_set(self, set_id) -> SearchSetView:
        """Run the one-query path over search set ``set_id`` from now on (``None``: the whole database) and return its view.  While a
        set is in use every result array is compact ([M]...) and every row argument and result is a position in the view
        (include/vq_amd_rows.h).  No library call when the set in use does not change; a change invalidates the similarities and
        scores the handle holds."""
        with self.lock:
            if set_id is None:
                if self._whole is None:
                    self._whole = whole_view(self)
                view = self._whole
            else:
                view = self._sets[set_id]
            if set_id != self._set_in_use:
                call("vq_db_rows_use", self._h, view.token)
                self._set_in_use, self._na = set_id, view.n
            return view

    def search_set_view(self, set_id) -> SearchSetView:
        """The view of a defined search set (``None``: the whole database) without selecting it: no library call, the set in use
        and the handle's results stay as they are."""
        with self.lock:
            if set_id is None:
                if self._whole is None:
                    self._whole = whole_view(self)
                return self._whole
            return self._sets[set_id]

    def drop_search_set(self, set_id):
        with self.lock:
            view = self._sets[set_id]
            call("vq_db_rows_drop", self._h, view.token)         # the set in use: VqError (VQ_E_STATE)
            del self._sets[set_id]

    @property
    def search_set_in_use(self):
        return self._set_in_use

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, feats: np.ndarray, clip_ids=None, present=None, device: int = 0, dtype=None) -> "FeatureDB":
        """Without ``dtype`` the block is stored as it comes if it is float32 / float64 and as float32 otherwise (float16 input
        included); ``dtype`` says how to store it -- ``np.float16`` keeps halves as they are and rounds anything else (upload)."""
        feats = np.asarray(feats)
        if feats.ndim != 4:
            raise ValueError("feats must be [N,S,E,D]")
        if dtype is None and feats.dtype not in (np.float32, np.float64):
            feats = feats.astype(np.float32)
        n, s, e, d = feats.shape
        db = cls(n, s, e, d, feats.dtype if dtype is None else dtype, device, clip_ids)
        db.upload(0, feats)
        if present is not None:
            db.set_present(present)
        return db

    @classmethod
    def from_records(cls, records: Iterable[Mapping], target_features: Mapping, streams: Sequence[str],
                     feature_name: str, dtype=np.float64, device: int = 0) -> "FeatureDB":
        """Regroup API records exactly like ticket.py:358-382 + the walk of ticket.py:146-160.

        Slot ``e`` of stream ``s`` is the e-th split of ``target_features[s]`` (dict order = the order
        ``np.dot`` results are summed in at ticket.py:156); clips are numbered in the order the
        reference first meets them (stream-major, split, record order).
        """
        splits = set()
        for st in target_features:
            splits.update(target_features[st].keys())
        cand = {st: {sp: {} for sp in splits} for st in streams}
        for tf in records:                                            # ticket.py:374-381
            st = tf["dnn_stream_id"]
            if st in streams and tf["name"] == feature_name and tf["dnn_stream_split"] in splits:
                cand[st][tf["dnn_stream_split"]][tf["video_clip_id"]] = tf["feature_vector"]
        stream_list = list(target_features.keys())                    # iteration order of ticket.py:146
        slot_splits = [list(target_features[st].keys()) for st in stream_list]
        n_slots = max((len(x) for x in slot_splits), default=0)
        order = {}
        for st, sps in zip(stream_list, slot_splits):                 # first-seen order, ticket.py:146-160
            for sp in sps:
                for clip in cand[st][sp]:
                    if clip not in order:
                        order[clip] = len(order)
        n = len(order)
        if n == 0 or n_slots == 0:
            raise ValueError("no candidate features match the target's streams/splits")
        dim = None
        for st, sps in zip(stream_list, slot_splits):
            for sp in sps:
                for vec in cand[st][sp].values():
                    dim = len(vec)
                    break
        # a float16 database is the float64 block rounded once (upload), never a double rounding through another type
        host_dtype = np.float64 if np.dtype(dtype) == np.float16 else dtype
        feats = np.zeros((n, len(stream_list), n_slots, dim), dtype=host_dtype)
        present = np.zeros((n, len(stream_list), n_slots), dtype=np.uint8)
        for si, (st, sps) in enumerate(zip(stream_list, slot_splits)):
            for ei, sp in enumerate(sps):
                d = cand[st][sp]
                if not d:
                    continue
                rows = np.fromiter((order[c] for c in d), dtype=np.int64, count=len(d))
                feats[rows, si, ei] = np.asarray(list(d.values()), dtype=host_dtype)
                present[rows, si, ei] = 1
        db = cls(n, len(stream_list), n_slots, dim, dtype, device,
                 np.fromiter(order.keys(), dtype=np.int64, count=n))
        db.stream_names = stream_list
        db.slot_splits = slot_splits
        db.upload(0, feats)
        if not present.all():
            db.set_present(present)
        return db

    @classmethod
    def from_store(cls, path: str, device: int = 0, row0: int = 0, rows: int | None = None,
                   chunk_rows: int = 16384) -> "FeatureDB":
        """Rows [row0, row0+rows) of a binary feature store (feature_store.py) -> resident DB; the memory-mapped block
        is uploaded in chunks of ``chunk_rows`` clips, so host memory stays bounded at any database size."""
        from .feature_store import open_store
        meta, feats, ids, present = open_store(path)
        n_all = feats.shape[0]
        rows = n_all - row0 if rows is None else int(rows)
        if row0 < 0 or rows <= 0 or row0 + rows > n_all:
            raise ValueError("rows [%d,%d) outside the store's %d clips" % (row0, row0 + rows, n_all))
        db = cls(rows, feats.shape[1], feats.shape[2], feats.shape[3], feats.dtype, device, ids[row0:row0 + rows])
        for r in range(0, rows, chunk_rows):
            k = min(chunk_rows, rows - r)
            db.upload(r, np.ascontiguousarray(feats[row0 + r:row0 + r + k]))
        if present is not None:
            db.set_present(np.ascontiguousarray(present[row0:row0 + rows]))
        db.stream_names = list(meta["streams"])
        db.slot_splits = [list(meta["splits"])] * len(meta["streams"])
        return db

    @classmethod
    def from_csv_tree(cls, features_dir: str, streams: Sequence[str] | None = None, clip_id_base: int = 0, dtype=np.float32, device: int = 0,
                      layout: str = "rows") -> "FeatureDB":
        """The reference's ``data/features`` tree (``<video>/<name ending in the split digit>/<stream>_<blob>_features.csv``) -> a
        resident database, the decimal text parsed ON THE DEVICE (:meth:`load_csv`): the rows, ids, presence mask, ``stream_names`` and
        ``slot_splits`` that ``feature_store.store_from_csv_tree`` + :meth:`from_store` give, bit for bit, without the interpreter
        converting a value (src/api/api_load_records.py:45-58) and without a store on disk.  Same walk: videos sorted by name, a
        video's clips in clip-number order, ids ``clip_id_base + row + 1``; a (clip, stream, split) without a row is absent and reads
        back as zeros.  Pass one indexes the files and keeps only their clip numbers; pass two loads them.  ``clips`` is the
        ``(video, clip)`` of every row; ``csv_host_fields`` counts the fields the host had to resolve.  ``layout="tiled"`` (fp32) tiles the
        block first, so the values land in their tiles.  A value that the database's type cannot hold (float16: |x| >= 65520) or that
        is no number raises ``ValueError`` naming file, line and field."""
        import os
        from .tsn import feature_csv
        streams = list(feature_csv.STREAM_MODES if streams is None else streams)
        per_video, all_splits, dim = [], set(), None
        for video in sorted(d for d in os.listdir(features_dir) if os.path.isdir(os.path.join(features_dir, d))):
            vdir = os.path.join(features_dir, video)
            by_split = {}
            for sd in sorted(d for d in os.listdir(vdir) if os.path.isdir(os.path.join(vdir, d))):
                split_path = os.path.join(vdir, sd)
                nsplit = int(split_path.rstrip("/")[-1])                      # feature_csv.read_split_dir
                per_stream = {}
                for entry in sorted(os.scandir(split_path), key=lambda e: e.name):
                    if entry.is_file() and entry.name.endswith('.csv') and not entry.name.startswith('.'):
                        meta, cl, d, _n = feature_csv.index_features(entry.path)
                        per_stream[meta["dnn_stream"]] = (cl, entry.path, d)
                by_split[nsplit] = per_stream
                all_splits.add(nsplit)
            clips = sorted({int(c) for ps in by_split.values() for (cl, _p, _d) in ps.values() for c in cl})
            per_video.append((video, clips, by_split))
            for ps in by_split.values():
                for (_cl, _p, d) in ps.values():
                    dim = d
        splits = sorted(all_splits)
        n = sum(len(c) for _v, c, _b in per_video)
        if n == 0:
            raise ValueError("no feature files under %s" % features_dir)
        present = np.zeros((n, len(streams), len(splits)), dtype=np.uint8)
        names, jobs = [], []
        row0 = 0
        for video, clips, by_split in per_video:
            local = {c: row0 + i for i, c in enumerate(clips)}
            names.extend((video, c) for c in clips)
            for ei, sp in enumerate(splits):
                for si, st in enumerate(streams):
                    if sp in by_split and st in by_split[sp]:
                        cl, path, _d = by_split[sp][st]
                        rows = np.array([local[int(c)] for c in cl], dtype=np.int64)
                        present[rows, si, ei] = 1
                        last = {r: i for i, r in enumerate(rows.tolist())}      # a clip number met twice in a file: its last row stays
                        if len(last) != rows.size:
                            rows[[i for i, r in enumerate(rows.tolist()) if last[r] != i]] = -1
                        jobs.append((path, si, ei, rows))
            row0 += len(clips)
        db = cls(n, len(streams), len(splits), dim, dtype, device, clip_id_base + np.arange(1, n + 1, dtype=np.int64))
        if layout != "rows":
            db.set_layout(layout)
        db.clips, db.csv_host_fields = names, 0
        if not present.all():
            # a new handle's block is not cleared and an absent slot reads back as zeros: clear the rows that lack one, then load
            lacking = np.flatnonzero(~present.reshape(n, -1).all(axis=1))
            for run in np.split(lacking, np.flatnonzero(np.diff(lacking) != 1) + 1):
                for r in range(int(run[0]), int(run[-1]) + 1, 4096):
                    db.upload(r, np.zeros((min(4096, int(run[-1]) + 1 - r), db.S, db.E, db.D), dtype=db.dtype))
        for path, si, ei, rows in jobs:
            with open(path, 'rb') as f:
                data = f.read()
            try:
                db.csv_host_fields += db.load_csv(data, si, ei, rows)
            except _lib.VqError as e:
                if e.code != -1:                                  # only VQ_E_INVALID is about the file's contents
                    raise
                raise ValueError("%s: %s" % (path, e)) from e
        if not present.all():
            db.set_present(present)
        db.stream_names = streams
        db.slot_splits = [list(splits)] * len(streams)
        return db

    @classmethod
    def synthetic(cls, n: int, n_streams: int, n_splits: int, dim: int = 1024, seed: int = 0,
                  scales: Sequence[float] = (4.0, 1.0), row0: int = 0, dtype=np.float32, device: int = 0,
                  clip_ids=None) -> "FeatureDB":
        """Rows generated on the device by the counter-based hash (oracle.sim_oracle.synth_features)."""
        db = cls(n, n_streams, n_splits, dim, dtype, device, clip_ids)
        sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float32))
        if sc.shape != (n_streams,):
            raise ValueError("scales must have one entry per stream")
        call("vq_db_generate", db._h, C.c_uint64(seed), row0, sc.ctypes.data_as(C.POINTER(C.c_float)))
        return db

    # ------------------------------------------------------------------ data movement
    def upload(self, row0: int, feats: np.ndarray):
        """Rows [row0, row0 + len(feats)) from the host, converted to the database's dtype.  Into a float16 database: round to nearest
        even; a finite value no half can hold raises ``ValueError`` (feature_store.to_float16)."""
        if self.dtype == np.float16:
            from .feature_store import to_float16
            feats = to_float16(feats)
        a = np.ascontiguousarray(feats, dtype=self.dtype)
        if a.shape[1:] != (self.S, self.E, self.D):
            raise ValueError("rows must be [n,%d,%d,%d]" % (self.S, self.E, self.D))
        call("vq_db_upload", self._h, int(row0), a.shape[0], _np_ptr(a))

    def load_csv(self, data, stream: int, split: int, rows, chunk_bytes: int = 0) -> int:
        """The values of one feature file (``data``: its bytes, header line included) into slot (``stream``, ``split``): data row i goes
        to DATABASE row ``rows[i]``, -1 skips it.  The text is parsed on the device (vq_db_load_csv, include/vq_amd_csv.h) into the
        database's dtype and layout; returns how many fields the host had to resolve.  ``VqError`` (VQ_E_INVALID) names line and field
        of a malformed value or of one a float16 database cannot hold; nothing is stored when ``rows`` names a row twice or outside the
        database, or its length or the file's dim do not match."""
        data = bytes(data)
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        host = C.c_int64()
        call("vq_db_load_csv", self._h, data, len(data), int(stream), int(split), _np_ptr(r) if r.size else None, int(r.size), int(chunk_bytes),
             C.byref(host))
        return int(host.value)

    def set_layout(self, layout: str):
        """"rows" ([N][S][E][D]) or "tiled" ([tile of 16 clips][S*E][D/4][clip][4]: the order in which every load of the scans
        takes whole lines; fp32 only, D = 1024, S <= 2, E <= 5).  In place, one sweep of the block: call once after loading."""
        call("vq_db_set_layout", self._h, {"rows": _lib.VQ_LAYOUT_ROWS, "tiled": _lib.VQ_LAYOUT_TILED}[layout])

    @property
    def layout(self) -> str:
        v = C.c_int32()
        call("vq_db_layout", self._h, C.byref(v))
        return "tiled" if v.value == _lib.VQ_LAYOUT_TILED else "rows"

    def adopt_device(self, dev_ptr: int, keepalive=None):
        """Use caller-owned device memory (e.g. a torch tensor holding all-gathered blocks)."""
        call("vq_db_adopt_device", self._h, C.c_void_p(dev_ptr))
        self._keepalive = keepalive

    def set_present(self, present):
        """The database's OWN presence mask [N,S,E] (None = dense).  Per-query restrictions go through
        :meth:`restrict_slots` and never change it."""
        if present is None:
            self.present = None
        else:
            p = np.ascontiguousarray(np.asarray(present).astype(np.uint8))
            if p.shape != (self.n, self.S, self.E):
                raise ValueError("present must be [N,S,E]")
            self.present = p
        self._slots_hidden = None
        call("vq_db_set_present", self._h, None if self.present is None else _np_ptr(self.present))

    def restrict_slots(self, slot_used):
        """Hide the (stream, split) slots a query's target lacks (the reference never visits them, ticket.py:146-148)
        for the scans that follow; ``None`` / all-true lifts the restriction.  The mask on the device is rebuilt from
        the database's own mask every time, so one ragged query leaves nothing behind for the next."""
        used = None if slot_used is None else np.asarray(slot_used, dtype=bool)
        if used is not None and used.shape != (self.S, self.E):
            raise ValueError("slot_used must be [S,E]")
        if used is not None and used.all():
            used = None
        hidden = None if used is None else ~used
        before = getattr(self, "_slots_hidden", None)
        if (hidden is None and before is None) or (hidden is not None and before is not None and (hidden == before).all()):
            return
        if hidden is None:
            effective = self.present
        else:
            base = self.present if self.present is not None else np.ones((self.n, self.S, self.E), dtype=np.uint8)
            effective = np.ascontiguousarray(base * used[None].astype(np.uint8))
        call("vq_db_set_present", self._h, None if effective is None else _np_ptr(effective))
        self._slots_hidden = hidden

    def set_stream(self, hip_stream: int):
        call("vq_db_set_stream", self._h, C.c_void_p(hip_stream))

    def feats_devptr(self) -> int:
        p = C.c_void_p()
        call("vq_db_feats_devptr", self._h, C.byref(p))
        return p.value

    def scores_devptr(self) -> int:
        p = C.c_void_p()
        call("vq_db_scores_devptr", self._h, C.byref(p))
        return p.value

    def avg_devptr(self) -> int:
        p = C.c_void_p()
        call("vq_db_avg_devptr", self._h, C.byref(p))
        return p.value

    def device_tensor(self, kind: str):
        """Zero-copy torch view of a result array in the library's device memory -- "avg" [N,S] f64, "ne" [N,S] i32, "scores"
        [N] f64 -- for collectives that take device tensors (RCCL all-gather of score slices).  The caller orders its use
        behind the scan (same stream as ``set_stream``)."""
        _lib.require_torch_runtime("FeatureDB.device_tensor")
        import torch
        n = self._na                                          # a search set in use: its M positions
        name, shape, typestr = {"avg": ("vq_db_avg_devptr", (n, self.S), "<f8"), "ne": ("vq_db_ne_devptr", (n, self.S), "<i4"),
                                "scores": ("vq_db_scores_devptr", (n,), "<f8")}[kind]
        p = C.c_void_p()
        call(name, self._h, C.byref(p))

        class _View:
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(p.value), False), "version": 2}
        return torch.as_tensor(_View(), device=torch.device("cuda", self.device))

    def read_rows(self, rows: Sequence[int]) -> np.ndarray:
        """Feature rows [L,S,E,D] back on the host (database dtype)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        out = np.empty((r.size, self.S, self.E, self.D), dtype=self.dtype)
        call("vq_db_read_rows", self._h, _np_ptr(r) if r.size else None, int(r.size), _np_ptr(out))
        return out

    def scores_at(self, rows: Sequence[int]) -> np.ndarray:
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        out = np.empty(r.size, dtype=np.float64)
        call("vq_db_read_scores_at", self._h, _np_ptr(r) if r.size else None, int(r.size), _np_ptr(out))
        return out

    # ------------------------------------------------------------------ query
    def set_query(self, t: np.ndarray):
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.shape != (self.S, self.E, self.D):
            raise ValueError("query must be [%d,%d,%d]" % (self.S, self.E, self.D))
        with self.lock:
            call("vq_db_set_query", self._h, _np_ptr(t))

    def set_query_from_row(self, row: int, want: bool = True):
        """t = r/(r.r) of a resident row (target_clip.py:311-313), computed on the device."""
        out = np.empty((self.S, self.E, self.D), dtype=np.float64) if want else None
        with self.lock:
            call("vq_db_set_query_from_row", self._h, int(row), _np_ptr(out) if want else None)
        return out

    def bootstrap_target(self, valid_rows: Sequence[int], invalid_rows: Sequence[int] = (), mu: float = 0.0,
                         set_query: bool = True) -> np.ndarray:
        """New query vectors [S,E,D] from user-validated resident clips (target_clip.py:161-261, closed forms on the
        device; see csrc/vq_boot.hip).  With ``set_query`` they become the query of the next scan."""
        v = np.ascontiguousarray(valid_rows, dtype=np.int64)
        iv = np.ascontiguousarray(invalid_rows, dtype=np.int64)
        out = np.empty((self.S, self.E, self.D), dtype=np.float64)
        with self.lock:
            call("vq_db_bootstrap_target", self._h, _np_ptr(v), int(v.size), _np_ptr(iv) if iv.size else None, int(iv.size), float(mu),
                 _np_ptr(out), 1 if set_query else 0)
        return out

    def scan(self, weights: Sequence[float] | None = None, keep_sims: bool = False):
        """One pass over the DB (ticket.py:120-163 [+ 165-180 when weights are given])."""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != (self.S,):
            raise ValueError("one weight per stream")
        with self.lock:
            call("vq_db_scan", self._h, _np_ptr(w) if w is not None else None, 1 if keep_sims else 0)

    def scan_batch(self, targets: np.ndarray, weights: np.ndarray, want: bool = True):
        """Q <= 16 queries in one pass over the database: targets [Q,S,E,D] fp64, weights [Q,S] -> scores [Q,N].  The dots
        run on the fp64 matrix cores, so the scores equal Q single scans to rounding (<= 1e-12), not bit for bit; the
        single-query state of the DB is left alone."""
        t = np.ascontiguousarray(targets, dtype=np.float64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if t.ndim != 4 or t.shape[1:] != (self.S, self.E, self.D) or w.shape != (t.shape[0], self.S):
            raise ValueError("targets must be [Q,%d,%d,%d] and weights [Q,%d]" % (self.S, self.E, self.D, self.S))
        out = np.empty((t.shape[0], self.n), dtype=np.float64) if want else None
        call("vq_db_scan_batch", self._h, t.shape[0], _np_ptr(t), _np_ptr(w), _np_ptr(out) if want else None)
        return out

    # ------------------------------------------------------------------ a query round in one call
    def _round_block(self) -> _RoundBlock:
        try:
            ptr, nbytes = self._round_pool["free"].pop()     # list.pop is atomic: two threads never take the same block
        except IndexError:
            p = C.c_void_p()
            nbytes = self._round_off[8]
            call("vq_host_alloc", C.byref(p), nbytes)
            ptr = p.value
        return _RoundBlock(ptr, nbytes, self._round_pool)

    def query_round(self, t: np.ndarray | None, weights=None, select=None) -> RoundResult:
        """ticket.py:120-180,311-356 as ONE call of the library (vq_db_query_round): one lock, one synchronisation, one copy back.
        ``t`` [S,E,D]: scan under this query (None: the similarities the handle holds); ``weights`` [S]: scores under them;
        ``select`` = (threshold, lower): the order-preserving partition.  Bit for bit what set_query / scan / similarities / rescore /
        scores / select return one by one (tested); the arrays are views of page-locked memory that stay valid as long as they live.
        The round and the fetch of a list longer than its 1024-row prefix run under ``self.lock``, which every method that replaces
        the handle's scores or selection lists takes: the lists are this round's whatever other threads ask of the handle."""
        blk = self._round_block()
        off = self._round_off
        raw = blk.bytes()
        S = self.S

        def view(piece, dtype, count, shape):
            return raw[off[piece]:off[piece] + count * dtype().itemsize].view(dtype).reshape(shape)
        flags = 0
        if t is not None:
            view(0, np.float64, S * self.E * self.D, (S, self.E, self.D))[...] = t
            flags |= 1
        if weights is not None:
            view(1, np.float64, S, (S,))[...] = weights
            flags |= 2
        th, lower = (float(select[0]), float(select[1])) if select is not None else (0.0, 0.0)
        if select is not None:
            flags |= 4
        # one lock from the round to the fetch of a list that outgrew its prefix: a selection, a top-k or a round of another thread on
        # this handle in between would replace (or invalidate) the lists on the device that the fetch copies
        with self.lock:
            n = self._na                                      # the block is laid out for N; a search set fills the first M of each array
            call("vq_db_query_round", self._h, C.c_void_p(blk.ptr), blk.nbytes, flags, th, lower)
            r = RoundResult()
            r.avg = view(2, np.float64, n * S, (n, S)) if t is not None else None
            r.n_e = view(3, np.int32, n * S, (n, S)) if t is not None else None
            r.scores = view(4, np.float64, n, (n,)) if weights is not None else None
            r.match_rows = r.near_rows = None
            r.near_argmax = -1
            if select is not None:
                res = view(5, np.int64, 4, (4,))
                nm, nn, r.near_argmax = int(res[0]), int(res[1]), int(res[2])
                if nm <= off[9] and nn <= off[9]:
                    r.match_rows = view(6, np.int64, nm, (nm,))
                    r.near_rows = view(7, np.int64, nn, (nn,))
                else:                                         # a list longer than its prefix: the full lists are still on the device
                    m = np.empty(nm, dtype=np.int64)
                    q = np.empty(nn, dtype=np.int64)
                    call("vq_db_select_fetch", self._h, _np_ptr(m) if nm else None, nm, _np_ptr(q) if nn else None, nn)
                    r.match_rows, r.near_rows = m, q
        return r

    # ------------------------------------------------------------------ up to 16 query rounds in one pass
    def batch_round_supported(self) -> bool:
        """Does this database meet the preconditions of the 16-query pass (include/vq_amd_rounds.h)?  The whole database only: the
        caller selects it first (``use_search_set(None)``)."""
        return self.D in (256, 512, 768, 1024) and self.S <= 8

    @staticmethod
    def _block_view(raw: np.ndarray, off):
        """view(piece, dtype, shape, first=0) over a block laid out by ``off``: ``shape`` elements of ``piece``, from its element
        ``first`` on."""
        def view(piece, dtype, shape, first=0):
            count, size = int(np.prod(shape)), np.dtype(dtype).itemsize
            lo = off[piece] + first * size
            return raw[lo:lo + count * size].view(dtype).reshape(shape)
        return view

    def _fill_round_inputs(self, view, Q: int, slots, w, bands, t=None) -> int:
        """The inputs of a batched round's block of ``Q`` queries: the targets (a round), and for the queries ``slots`` their weights
        (padded to 8) and bands; ``slots`` indexes the rows of [Q, ...] arrays.  Returns the partition flag the bands ask for."""
        if t is not None:
            view(0, np.float64, (Q, self.S, self.E, self.D))[...] = t
        wv, bv = view(1, np.float64, (Q, 8)), view(2, np.float64, (Q, 2))
        wv[...] = 0.0
        bv[...] = 0.0
        wv[slots, :self.S] = w
        if bands is None:
            return 0
        bv[slots] = bands
        return _lib.VQ_BROUND_SELECT

    def _partition_decoder(self, view, off, Q: int):
        """decode(r, q, have): the partition of query q of the last batched round into ``r`` from the block's results and prefixes;
        a list longer than its prefix is fetched (the full lists are still on the device).  Call under ``self.lock``."""
        res = view(6, np.int64, (Q, 4))
        prefix = off[10]
        pre_m, pre_n = view(7, np.int64, (Q, prefix)), view(8, np.int64, (Q, prefix))

        def decode(r, q, have):
            r.match_rows = r.near_rows = None
            r.near_argmax = -1
            if not have:
                return
            nm, nn, r.near_argmax = int(res[q, 0]), int(res[q, 1]), int(res[q, 2])
            if nm <= prefix and nn <= prefix:
                r.match_rows, r.near_rows = pre_m[q, :nm], pre_n[q, :nn]
            else:
                m = np.empty(nm, dtype=np.int64)
                k = np.empty(nn, dtype=np.int64)
                call("vq_db_batch_round_fetch", self._h, q, _np_ptr(m) if nm else None, nm, _np_ptr(k) if nn else None, nn)
                r.match_rows, r.near_rows = m, k
        return decode

    def _round_flags(self, want_avg: bool, want_scores: bool, timed: bool) -> int:
        return (_lib.VQ_BROUND_SCORES if want_scores else 0) | (_lib.VQ_BROUND_AVG if want_avg else 0) | (_lib.VQ_BROUND_TIMED if timed else 0)

    def _batch_round_block(self, q: int):
        """(block, offsets) for a batched round of ``q`` queries: a page-locked block from the pool of its size (_RoundBlock's pooling,
        one pool per number of queries -- the layout depends on it)."""
        pools = self.__dict__.setdefault("_batch_round_pools", {})
        if q not in pools:
            off = (C.c_int64 * 12)()
            call("vq_db_batch_round_layout", self._h, q, off)
            pools[q] = ([int(v) for v in off], {"free": [], "closed": False})
        off, pool = pools[q]
        if pool["free"]:
            ptr, nbytes = pool["free"].pop()
        else:
            p = C.c_void_p()
            nbytes = off[9]
            call("vq_host_alloc", C.byref(p), nbytes)
            ptr = p.value
        return _RoundBlock(ptr, nbytes, pool), off

    def query_round_batch(self, targets: np.ndarray, weights: np.ndarray, selects=None, want_avg: bool = True, timed: bool = False,
                          want_scores: bool = True) -> list:
        """Up to 16 query rounds in ONE read of the database (vq_db_query_round_batch): ``targets`` [Q,S,E,D] fp64, ``weights`` [Q,S],
        ``selects`` [Q,2] = (threshold, lower) per query or None.  One :class:`RoundResult` per query with the fields
        :meth:`query_round` fills: ``avg`` [N,S] (None without ``want_avg``), ``n_e`` [N,S] (ONE array shared by all results: it does not
        depend on the query), ``scores`` [N], ``match_rows`` / ``near_rows`` / ``near_argmax`` (with ``selects``).  The scores are
        :meth:`scan_batch`'s bit for bit, scores and avg the one-query round's to rounding (<= 1e-12); the partition is exact on the
        returned scores.  The arrays are views of one pooled page-locked block that lives as long as they do; a list longer than
        the prefix is fetched.  The whole database only (a search set in use: ``VqError``); the one-query state of the handle is left
        alone.  ``timed``: :meth:`batch_round_times` then gives the split of the call.  ``want_scores=False``: the scores are not
        copied back (``scores`` is None); they stay on the device for :meth:`batch_round_topk`, :meth:`batch_round_rescore` and
        ``vq_db_batch_scores_devptr``, so a ranked search never moves an N-sized array."""
        t = np.asarray(targets, dtype=np.float64)
        w = np.asarray(weights, dtype=np.float64)
        if t.ndim != 4 or t.shape[1:] != (self.S, self.E, self.D) or w.shape != (t.shape[0], self.S):
            raise ValueError("targets must be [Q,%d,%d,%d] and weights [Q,%d]" % (self.S, self.E, self.D, self.S))
        Q = int(t.shape[0])
        bands = None if selects is None else np.asarray(selects, dtype=np.float64)
        if bands is not None and bands.shape != (Q, 2):
            raise ValueError("selects must be [Q,2]: (threshold, lower) per query")
        if not 1 <= Q <= 16:
            call("vq_db_batch_round_layout", self._h, Q, (C.c_int64 * 12)())      # the library's own refusal (VqError)
        with self.lock:
            self._bround_last = None                          # the round before is gone (its block may serve this one)
            blk, off = self._batch_round_block(Q)
            view = self._block_view(blk.bytes(), off)
            n, S = self.n, self.S
            flags = self._round_flags(want_avg, want_scores, timed) | self._fill_round_inputs(view, Q, slice(None), w, bands, t)
            call("vq_db_query_round_batch", self._h, Q, C.c_void_p(blk.ptr), blk.nbytes, flags)
            n_e = view(3, np.int32, (n, S)) if want_avg else None
            avg = view(4, np.float64, (Q, n, S)) if want_avg else None
            scores = view(5, np.float64, (Q, n)) if want_scores else None
            decode = self._partition_decoder(view, off, Q)
            out = []
            for q in range(Q):
                r = RoundResult()
                r.avg = avg[q] if want_avg else None
                r.n_e = n_e
                r.scores = scores[q] if want_scores else None
                decode(r, q, bands is not None)
                out.append(r)
            # what batch_round_rescore lays its block out by, and the round's avg / n_e its results carry
            self._bround_last = (Q, off, [q * n for q in range(Q + 1)], None, [(r.avg, r.n_e) for r in out])
            return out

    def query_round_batch_sets(self, targets: np.ndarray, weights: np.ndarray, set_ids, selects=None, want_avg: bool = True,
                               timed: bool = False, want_scores: bool = True) -> list:
        """:meth:`query_round_batch` with a search set per query (vq_db_query_round_views, include/vq_amd_round_views.h): ONE read of
        the UNION of the sets, every query scored, averaged and partitioned over its own set only.  ``set_ids[q]`` is a defined search
        set id, or ``None`` for the whole database.  One :class:`RoundResult` per query: ``avg`` [M_q,S], ``n_e`` [M_q,S] and ``scores``
        [M_q] are compact (entry i belongs to row ``rows[i]`` of the set's view) and every row in ``match_rows`` / ``near_rows`` /
        ``near_argmax`` is a position in that view, as under :meth:`use_search_set`.  avg and scores have the bits
        :meth:`query_round_batch` gives the same (clip, query slot) on this handle.  The set in use and the one-query state of the
        handle are left alone.  :attr:`last_view_round_union` then says what the pass read.  ``want_scores=False``: as for
        :meth:`query_round_batch` (``scores`` is None, the scores stay on the device)."""
        t = np.asarray(targets, dtype=np.float64)
        w = np.asarray(weights, dtype=np.float64)
        if t.ndim != 4 or t.shape[1:] != (self.S, self.E, self.D) or w.shape != (t.shape[0], self.S):
            raise ValueError("targets must be [Q,%d,%d,%d] and weights [Q,%d]" % (self.S, self.E, self.D, self.S))
        Q = int(t.shape[0])
        set_ids = list(set_ids)
        if len(set_ids) != Q:
            raise ValueError("one search set id (or None) per query")
        bands = None if selects is None else np.asarray(selects, dtype=np.float64)
        if bands is not None and bands.shape != (Q, 2):
            raise ValueError("selects must be [Q,2]: (threshold, lower) per query")
        with self.lock:
            self._bround_last = None                          # the round before is gone (its block may serve this one)
            tokens = (C.c_int32 * max(Q, 1))()
            for q, sid in enumerate(set_ids):
                if sid is not None and not self.has_search_set(sid):
                    raise _lib.VqError(-1, "query %d: search set %r is not defined on this database" % (q, sid))
                tokens[q] = -1 if sid is None else self._sets[sid].token
            off, start = (C.c_int64 * 12)(), (C.c_int64 * 17)()
            call("vq_db_view_round_layout", self._h, Q, tokens, off, start)          # Q outside [1, 16]: the library's own refusal
            off, start = [int(v) for v in off], [int(v) for v in start]
            blk = self._pooled_block("_view_round_pools", off[9])                     # pooled by size: the layout depends on the sets
            view = self._block_view(blk.bytes(), off)
            S = self.S
            flags = self._round_flags(want_avg, want_scores, timed) | self._fill_round_inputs(view, Q, slice(None), w, bands, t)
            call("vq_db_query_round_views", self._h, Q, tokens, C.c_void_p(blk.ptr), blk.nbytes, flags)
            decode = self._partition_decoder(view, off, Q)
            out = []
            for q in range(Q):
                m = start[q + 1] - start[q]
                r = RoundResult()
                r.avg = view(4, np.float64, (m, S), start[q] * S) if want_avg else None
                r.n_e = view(3, np.int32, (m, S), start[q] * S) if want_avg else None
                r.scores = view(5, np.float64, (m,), start[q]) if want_scores else None
                decode(r, q, bands is not None)
                out.append(r)
            self._bround_last = (Q, off, start, blk._pool, [(r.avg, r.n_e) for r in out])       # as after query_round_batch
            return out

    @property
    def last_view_round_union(self):
        """(rows, tiles) of the last :meth:`query_round_batch_sets`: the rows in the union of its sets, and the tiles of 16 rows the
        union touches (what the pass read of a tiled database)."""
        rows, tiles = C.c_int64(), C.c_int64()
        call("vq_db_view_round_union", self._h, C.byref(rows), C.byref(tiles))
        return int(rows.value), int(tiles.value)

    def batch_round_times(self):
        """(pass, selection, copy-back) in ms of the last ``query_round_batch(..., timed=True)``: device time between HIP events."""
        ms = (C.c_float * 3)()
        call("vq_db_batch_round_times", self._h, ms)
        return tuple(float(v) for v in ms)

    # ------------------------------------------------------------------ weight fits and re-weighting on a batched round's device data
    def _pooled_block(self, name: str, nbytes: int) -> _RoundBlock:
        """A page-locked block of at least ``nbytes`` from the pool ``name`` keeps by size (rounded up to 64 KiB)."""
        pools = self.__dict__.setdefault(name, {})
        nbytes = (max(nbytes, 1) + 65535) // 65536 * 65536
        if nbytes not in pools and len(pools) >= 8:               # many sizes: the idle blocks of the old ones go
            for size in list(pools):
                old = pools.pop(size)
                old["closed"] = True
                while old["free"]:
                    _lib.load().vq_host_free(C.c_void_p(old["free"].pop()[0]))
        pool = pools.setdefault(nbytes, {"free": [], "closed": False})
        if pool["free"]:
            ptr, _ = pool["free"].pop()
        else:
            p = C.c_void_p()
            call("vq_host_alloc", C.byref(p), nbytes)
            ptr = p.value
        return _RoundBlock(ptr, nbytes, pool)

    def batch_round_fit(self, queries, rows, labels, w_grids, th_grids, ballasts) -> list:
        """hyperparameter.py:57-64 for several queries of the LAST batched round (either kind) in one call and one launch
        (vq_db_batch_round_fit, include/vq_amd_round_fit.h), on the averaged similarities that round left on the device.  Per entry
        i: ``queries[i]`` the query's index in that round, ``rows[i]`` / ``labels[i]`` its labelled rows (positions in the query's
        view, as in the round's results) and their labels, ``w_grids[i]`` [G,S], ``th_grids[i]`` [T] and ``ballasts[i]``; G and T are
        common to the call.  Returns one [G,T] array per entry: the raw sums of :meth:`loss_surface` on the same similarities, bit
        for bit, for any number of labels (the caller divides by it).  An entry without labels gets None."""
        queries = [int(q) for q in queries]
        k = len(queries)
        if not (k and len(rows) == len(labels) == len(w_grids) == len(th_grids) == len(ballasts) == k) or len(set(queries)) != k:
            raise ValueError("one rows / labels / w_grid / th_grid / ballast per query, every query once")
        wg = [np.asarray(w, dtype=np.float64) for w in w_grids]
        th = [np.asarray(t, dtype=np.float64).reshape(-1) for t in th_grids]
        rs = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
        ys = [np.asarray(y, dtype=np.float64).reshape(-1) for y in labels]
        G, T = int(wg[0].shape[0]), int(th[0].size)
        if any(w.ndim != 2 or w.shape != (G, self.S) for w in wg) or any(t.size != T for t in th) or any(r.shape != y.shape for r, y in zip(rs, ys)):
            raise ValueError("w_grids must be [G,%d] and th_grids [T] with one G and T for the call, and one label per row" % self.S)
        if min(queries) < 0:
            raise ValueError("a query is its index in the last batched round")
        with self.lock:
            Q = max(queries) + 1                              # slot q of the block = query q of the round; the library refuses what that round lacks
            order = sorted(range(k), key=lambda i: queries[i])
            total = int(sum(r.size for r in rs))
            off = (C.c_int64 * 8)()
            call("vq_db_batch_fit_layout", self._h, Q, G, T, total, off)
            off = [int(v) for v in off]
            blk = self._pooled_block("_fit_pools", off[7])
            view = self._block_view(blk.bytes(), off)
            w_in, th_in, b_in, l_in = view(0, np.float64, (Q, G, 8)), view(1, np.float64, (Q, T)), view(2, np.float64, (Q,)), view(3, np.int64, (Q,))
            r_in, y_in = view(4, np.int64, (total,)), view(5, np.float64, (total,))
            w_in[...] = 0.0
            th_in[...] = 0.0
            b_in[...] = 0.0
            l_in[...] = 0
            at = 0
            for i in order:
                q = queries[i]
                w_in[q, :, :self.S], th_in[q], b_in[q], l_in[q] = wg[i], th[i], float(ballasts[i]), rs[i].size
                r_in[at:at + rs[i].size], y_in[at:at + rs[i].size] = rs[i], ys[i]
                at += rs[i].size
            call("vq_db_batch_round_fit", self._h, Q, G, T, total, C.c_void_p(blk.ptr), blk.nbytes)
            surface = view(6, np.float64, (Q, G, T))
            return [surface[queries[i]] if rs[i].size else None for i in range(k)]

    def batch_round_grid(self, queries, rows, w_grids) -> list:
        """hyperparameter.py:57-58 on chosen rows for several queries of the LAST batched round (either kind) in one call and one
        launch (vq_db_batch_round_grid, include/vq_amd_round_grid.h): per entry i, the scores of ``rows[i]`` (positions in the view
        of query ``queries[i]`` of that round, as in its results; a row may repeat) under each weight of ``w_grids[i]`` [G,S], on the
        averaged similarities the round left on the device; G is common to the call.  Returns one [G, L_i] array per entry -- the bits
        of :meth:`scores_grid` on the same similarities, and with the round's (or the rescore's) weights the bits of that round's own
        scores at those rows -- and None for an entry without rows.  What a row-sharded database combines into its weight fit."""
        queries = [int(q) for q in queries]
        k = len(queries)
        if not (k and len(rows) == len(w_grids) == k) or len(set(queries)) != k:
            raise ValueError("one rows / w_grid per query, every query once")
        wg = [np.asarray(w, dtype=np.float64) for w in w_grids]
        rs = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
        G = int(wg[0].shape[0]) if wg[0].ndim == 2 else -1
        if any(w.ndim != 2 or w.shape != (G, self.S) for w in wg):
            raise ValueError("w_grids must be [G,%d] with one G for the call" % self.S)
        if min(queries) < 0:
            raise ValueError("a query is its index in the last batched round")
        with self.lock:
            Q = max(queries) + 1                              # slot q of the block = query q of the round; the library refuses what that round lacks
            order = sorted(range(k), key=lambda i: queries[i])
            total = int(sum(r.size for r in rs))
            off = (C.c_int64 * 5)()
            call("vq_db_batch_grid_layout", self._h, Q, G, total, off)
            off = [int(v) for v in off]
            blk = self._pooled_block("_grid_pools", off[4])
            view = self._block_view(blk.bytes(), off)
            w_in, l_in, r_in = view(0, np.float64, (Q, G, 8)), view(1, np.int64, (Q,)), view(2, np.int64, (total,))
            w_in[...] = 0.0
            l_in[...] = 0
            at, first = 0, {}
            for i in order:
                q = queries[i]
                w_in[q, :, :self.S], l_in[q] = wg[i], rs[i].size
                r_in[at:at + rs[i].size] = rs[i]
                first[i] = at
                at += rs[i].size
            call("vq_db_batch_round_grid", self._h, Q, G, total, C.c_void_p(blk.ptr), blk.nbytes)
            return [view(3, np.float64, (G, rs[i].size), G * first[i]) if rs[i].size else None for i in range(k)]

    def batch_round_avg_rows(self, queries, rows) -> list:
        """The averaged similarities of chosen rows of several queries of the LAST batched round (either kind) in one call and one
        launch (vq_db_batch_round_avg_rows, include/vq_amd_round_shard.h): per entry i, ``avg[rows[i]]`` of query ``queries[i]`` of that
        round (positions in the query's view, as in its results; a row may repeat) as the round left them on the device -- copies,
        bit for bit, NaN payloads and the sign of zero included.  Returns one [L_i, S] array per entry, None for an entry without
        rows.  What the ranks of a row-sharded database exchange in front of :meth:`batch_round_update_given`."""
        queries = [int(q) for q in queries]
        k = len(queries)
        if not (k and len(rows) == k) or len(set(queries)) != k:
            raise ValueError("one list of rows per query, every query once")
        rs = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
        if min(queries) < 0:
            raise ValueError("a query is its index in the last batched round")
        with self.lock:
            Q = max(queries) + 1                              # slot q of the block = query q of the round; the library refuses what that round lacks
            order = sorted(range(k), key=lambda i: queries[i])
            total = int(sum(r.size for r in rs))
            off = (C.c_int64 * 4)()
            call("vq_db_batch_avg_rows_layout", self._h, Q, total, off)
            off = [int(v) for v in off]
            blk = self._pooled_block("_grid_pools", off[3])
            view = self._block_view(blk.bytes(), off)
            l_in, r_in = view(0, np.int64, (Q,)), view(1, np.int64, (total,))
            l_in[...] = 0
            at, first = 0, {}
            for i in order:
                l_in[queries[i]] = rs[i].size
                r_in[at:at + rs[i].size] = rs[i]
                first[i] = at
                at += rs[i].size
            call("vq_db_batch_round_avg_rows", self._h, Q, total, C.c_void_p(blk.ptr), blk.nbytes)
            return [view(2, np.float64, (rs[i].size, self.S), self.S * first[i]) if rs[i].size else None for i in range(k)]

    # ------------------------------------------------------------------ the bootstrapped targets of a group of tickets
    def batch_targets_lds_rows(self) -> int:
        """The largest draw (rows) whose systems ``batch_targets`` solves in a workgroup's local memory; longer draws solve in a
        scratch area in device memory (the library's constant, read through vq_db_batch_targets_layout)."""
        off = (C.c_int64 * 11)()
        call("vq_db_batch_targets_layout", self._h, 1, 1, 1, 1, off)
        return int(off[10])

    def batch_targets(self, pools, draws, mus, previous=None, keeps=None) -> list:
        """Target bootstrapping (target_clip.py:26-82) for up to 16 queries in ONE call (vq_db_batch_targets,
        include/vq_amd_round_targets.h).  Per query q: ``pools[q]`` = (valid_rows, invalid_rows), the database rows of its validated
        matches and non-matches; ``draws[q]`` = a list of (picked_valid, picked_invalid), positions into those two lists in the row
        order of the problem (``target_clip.draw_indices``); ``mus[q]``; and, to blend, ``previous[q]`` [S,E,D] with ``keeps[q]``
        (target = keep * target + (1 - keep) * previous).  Returns one [S,E,D] array per query: the mean over its draws of what
        :meth:`bootstrap_target` gives on each draw's rows, bit for bit (numpy's mean over axis 0; one draw: that draw's target).
        A singular system in a query raises ``VqError`` (VQ_E_INVALID) for the first such query, naming it; the handle's query,
        scores, last batched round and search set in use are left alone."""
        status, targets = self._batch_targets_raw(pools, draws, mus, previous, keeps)
        for q in range(len(targets)):
            if status[q, 0] != 0:
                raise _lib.VqError(-1, "query %d, draw %d: problem %d: singular system (linearly dependent validated clips) -- numpy.linalg.inv "
                                   "raises here too" % (q, int(status[q, 1]), int(status[q, 2])))
        return targets

    def _batch_targets_raw(self, pools, draws, mus, previous=None, keeps=None):
        """:meth:`batch_targets` up to the library's answer: (status [Q,4] int32 -- 0 solved / 1 singular, the first failing draw, its
        slot -- and the list of [S,E,D] targets; the target of a query with a status holds no result)."""
        Q = len(pools)
        if not Q or len(draws) != Q or len(mus) != Q or (previous is not None and len(previous) != Q) or (keeps is not None and len(keeps) != Q):
            raise ValueError("one pool, one list of draws and one mu per query (and one previous / keep when given)")
        valid = [np.asarray(p[0], dtype=np.int64).reshape(-1) for p in pools]
        invalid = [np.asarray(p[1], dtype=np.int64).reshape(-1) for p in pools]
        picks = [[(np.asarray(pv, dtype=np.int32).reshape(-1), np.asarray(pi, dtype=np.int32).reshape(-1)) for pv, pi in ds] for ds in draws]
        before = [None if previous is None or previous[q] is None else np.asarray(previous[q], dtype=np.float64) for q in range(Q)]
        if any(b is not None and b.shape != (self.S, self.E, self.D) for b in before):
            raise ValueError("previous targets must be [%d,%d,%d]" % (self.S, self.E, self.D))
        if any(b is not None and (keeps is None or keeps[q] is None) for q, b in enumerate(before)):
            raise ValueError("a previous target needs its keep")
        n_rows = int(sum(v.size + i.size for v, i in zip(valid, invalid)))
        n_draws = int(sum(len(ds) for ds in picks))
        n_entries = int(sum(pv.size + pi.size for ds in picks for pv, pi in ds))
        with self.lock:
            off = (C.c_int64 * 11)()
            call("vq_db_batch_targets_layout", self._h, Q, n_rows, n_draws, n_entries, off)
            off = [int(v) for v in off]
            blk = self._pooled_block("_target_pools", off[9])
            view = self._block_view(blk.bytes(), off)
            q_in, p_in = view(0, np.int32, (Q, 8)), view(1, np.float64, (Q, 4))
            r_in, d_in, e_in = view(2, np.int64, (n_rows,)), view(3, np.int32, (n_draws, 2)), view(4, np.int32, (n_entries,))
            prev_in = view(6, np.float64, (Q, self.S, self.E, self.D))
            q_in[...] = 0
            p_in[...] = 0.0
            r_at = d_at = e_at = 0
            for q in range(Q):
                m, n = valid[q].size, invalid[q].size
                q_in[q, :4] = (m + n, m, len(picks[q]), 0 if before[q] is None else 1)
                p_in[q, 0] = float(mus[q])
                if before[q] is not None:
                    keep = keeps[q]
                    p_in[q, 1], p_in[q, 2] = keep, (1 - keep)
                    prev_in[q] = before[q]
                r_in[r_at:r_at + m], r_in[r_at + m:r_at + m + n] = valid[q], invalid[q]
                r_at += m + n
                for pv, pi in picks[q]:
                    d_in[d_at] = (pv.size + pi.size, pv.size)
                    e_in[e_at:e_at + pv.size] = pv
                    e_in[e_at + pv.size:e_at + pv.size + pi.size] = pi + m
                    d_at += 1
                    e_at += pv.size + pi.size
            call("vq_db_batch_targets", self._h, Q, n_rows, n_draws, n_entries, C.c_void_p(blk.ptr), blk.nbytes)
            status = view(7, np.int32, (Q, 4))
            target = view(8, np.float64, (Q, self.S, self.E, self.D))
            return status, [target[q] for q in range(Q)]

    def batch_round_rescore(self, queries, weights, selects=None) -> list:
        """compute_matches.py:77 and ticket.py:311-356 for several queries of the LAST batched round (either kind) in one call
        (vq_db_batch_round_rescore): query ``queries[i]`` of that round is rescored under ``weights[i]`` [S] on the averaged
        similarities the round left on the device and, with ``selects`` [k,2] = (threshold, lower), partitioned again.  One
        :class:`RoundResult` per entry: ``scores`` (the bits of :meth:`rescore` + :meth:`scores` on the same similarities),
        ``match_rows`` / ``near_rows`` / ``near_argmax`` (those of :meth:`select` on them), ``avg`` and ``n_e`` the round's own.  The
        round's other queries keep their scores and lists on the device."""
        queries = [int(q) for q in queries]
        k = len(queries)
        w = np.asarray(weights, dtype=np.float64)
        bands = None if selects is None else np.asarray(selects, dtype=np.float64)
        if not k or len(set(queries)) != k or w.shape != (k, self.S) or (bands is not None and bands.shape != (k, 2)):
            raise ValueError("weights must be [k,%d] and selects [k,2] for k distinct queries" % self.S)
        if min(queries) < 0 or max(queries) >= 16:
            raise ValueError("a query is its index in the last batched round")
        flags = _lib.VQ_BROUND_SCORES | (_lib.VQ_BROUND_SELECT if bands is not None else 0)
        with self.lock:
            last = getattr(self, "_bround_last", None)
            if last is None or max(queries) >= last[0]:
                # no batched round, or a query it did not have: the library's own refusal (VQ_E_STATE), which reads nothing of the block
                blk = self._pooled_block("_fit_pools", 64)
                call("vq_db_batch_round_rescore", self._h, sum(1 << q for q in queries), C.c_void_p(blk.ptr), blk.nbytes, flags)
                raise _lib.VqError(-4, "the last batched round does not have queries %r" % (queries,))
            Q, off, start, pool, sims = last
            blk = self._batch_round_block(Q)[0] if pool is None else self._pooled_block("_view_round_pools", off[9])
            view = self._block_view(blk.bytes(), off)
            self._fill_round_inputs(view, Q, queries, w, bands)
            call("vq_db_batch_round_rescore", self._h, sum(1 << q for q in queries), C.c_void_p(blk.ptr), blk.nbytes, flags)
            decode = self._partition_decoder(view, off, Q)
            out = []
            for q in queries:
                r = RoundResult()
                r.avg, r.n_e = sims[q]
                r.scores = view(5, np.float64, (start[q + 1] - start[q],), start[q])
                decode(r, q, bands is not None)
                out.append(r)
            return out

    def batch_round_update(self, queries, rows, labels, w_grids, th_grids, ballasts, seconds, eps, reaches, user_rows, want_scores: bool = True,
                           want_surface: bool = False, surfaces=None) -> list:
        """The whole weight update of several queries of the LAST batched round (either kind) in ONE call (vq_db_batch_round_update,
        include/vq_amd_round_update.h): :meth:`batch_round_fit`, ``Hyperparameter._pick_exact`` of every surface divided by its number
        of labels, :meth:`batch_round_rescore` under the picked weights, the review band and the partition, chained on the device.
        Per entry i, beside the arguments of :meth:`batch_round_fit`: ``seconds[i]`` the column of ``w_grids[i]`` that carries the
        grid, ``eps`` (one float, or one per entry: COMPUTE_EPS), ``reaches[i]`` how far below the threshold the band reaches
        (``near_miss_default`` of a revise ticket) or ``None`` for a finalize ticket, whose reach comes from the lowest score at
        ``user_rows[i]`` (positions in the query's view; ``lowest_scoring_user_match``).  ``surfaces``: one raw [G,T] surface per entry
        instead of the fit (``rows`` is then ignored and ``labels[i]`` may be the NUMBER of labels: it is still the divisor).
        Returns one :class:`UpdateResult` per entry: scores (None without ``want_scores``; they stay on the device), partition, ``avg``
        and ``n_e`` as :meth:`batch_round_rescore` gives them under ``w`` and ``band``; the pick has the bits of ``_pick_exact``, ``band``
        those of the host's expressions over the returned scores.  ``surface`` is the fit's own (``want_surface``) or None."""
        return self._batch_update(queries, rows, labels, w_grids, th_grids, ballasts, seconds, eps, reaches, user_rows, want_scores, want_surface,
                                  surfaces, tables=False)

    def batch_round_update_given(self, queries, labels, label_avgs, w_grids, th_grids, ballasts, seconds, eps, reaches, user_avgs,
                                 want_scores: bool = True, want_surface: bool = False) -> list:
        """:meth:`batch_round_update` with the labelled and the user rows' averaged similarities GIVEN instead of read from the round
        (vq_db_batch_round_update_given, include/vq_amd_round_shard.h): ``label_avgs[i]`` [L_i, S] in label order and ``user_avgs[i]``
        [U_i, S] (or None) are what :meth:`batch_round_avg_rows` returns for those rows -- on this handle or, for a row-sharded
        database, put together from the handles that hold them.  ``L_i`` is the number of labels of the WHOLE database: the divisor.
        The surface, the pick, ``lowest`` and the band are functions of the tables alone, so every handle fed the same tables picks
        the same; the rescore and the partition are this handle's own rows'.  Fed the tables of its own rows the call returns what
        :meth:`batch_round_update` returns, bit for bit."""
        return self._batch_update(queries, label_avgs, labels, w_grids, th_grids, ballasts, seconds, eps, reaches, user_avgs, want_scores,
                                  want_surface, None, tables=True)

    def _batch_update(self, queries, rows, labels, w_grids, th_grids, ballasts, seconds, eps, reaches, user_rows, want_scores, want_surface,
                      surfaces, tables):
        """The two update calls: ``tables`` says whether ``rows`` / ``user_rows`` carry positions (int64) or [., S] averaged similarities."""
        queries = [int(q) for q in queries]
        k = len(queries)
        given = surfaces is not None
        row_t, width = (np.float64, self.S) if tables else (np.int64, 1)
        eps = [float(eps)] * k if np.ndim(eps) == 0 else [float(e) for e in eps]
        if not (k and len(rows) == len(labels) == len(w_grids) == len(th_grids) == len(ballasts) == len(seconds) == len(eps) == len(reaches)
                == len(user_rows) == k) or len(set(queries)) != k or (given and (len(surfaces) != k or want_surface)):
            raise ValueError("one rows / labels / w_grid / th_grid / ballast / second / reach / user_rows (and surface) per query, every query once")
        wg = [np.asarray(w, dtype=np.float64) for w in w_grids]
        th = [np.asarray(t, dtype=np.float64).reshape(-1) for t in th_grids]
        if given:
            counts = [int(y) if np.ndim(y) == 0 else len(y) for y in labels]
            rs, ys = [np.zeros(0, dtype=np.int64)] * k, [np.zeros(0)] * k
        else:
            rs = [np.asarray(r, dtype=row_t).reshape(-1) for r in rows]
            ys = [np.asarray(y, dtype=np.float64).reshape(-1) for y in labels]
            counts = [r.size // width for r in rs]
        us = [np.zeros(0, dtype=row_t) if u is None else np.asarray(u, dtype=row_t).reshape(-1) for u in user_rows]
        G, T = int(wg[0].shape[0]), int(th[0].size)
        if any(w.ndim != 2 or w.shape != (G, self.S) for w in wg) or any(t.size != T for t in th) or \
                any(r.size != y.size * width for r, y in zip(rs, ys)) or any(u.size % width for u in us):
            raise ValueError("w_grids must be [G,%d] and th_grids [T] with one G and T for the call, and one label per row%s"
                             % (self.S, " of [., %d] averaged similarities" % self.S if tables else ""))
        sf = [np.asarray(f, dtype=np.float64) for f in surfaces] if given else None
        if given and any(f.shape != (G, T) for f in sf):
            raise ValueError("surfaces must be [G,T]")
        if min(queries) < 0 or max(queries) >= 16:
            raise ValueError("a query is its index in the last batched round")
        flags = _lib.VQ_BROUND_SELECT | (_lib.VQ_BROUND_SCORES if want_scores else 0) | (_lib.VQ_BUPDATE_SURFACE if want_surface else 0) \
            | (_lib.VQ_BUPDATE_GIVEN_SURFACE if given else 0)
        with self.lock:
            Q = max(queries) + 1                              # slot q of the block = query q of the round; the library refuses what that round lacks
            order = sorted(range(k), key=lambda i: queries[i])
            total, total_u = int(sum(y.size for y in ys)), int(sum(u.size for u in us)) // width
            off = (C.c_int64 * 16)()
            call("vq_db_batch_update_given_layout" if tables else "vq_db_batch_update_layout", self._h, Q, G, T, total, total_u, off)
            off = [int(v) for v in off]
            ublk = self._pooled_block("_update_pools", off[15])
            view = self._block_view(ublk.bytes(), off)
            ublk.bytes()[:off[6]] = 0
            ublk.bytes()[off[7]:off[15]] = 0
            w_in, th_in, b_in, l_in = view(0, np.float64, (Q, G, 8)), view(1, np.float64, (Q, T)), view(2, np.float64, (Q,)), view(3, np.int64, (Q,))
            r_in, y_in, surface = view(4, row_t, (total * width,)), view(5, np.float64, (total,)), view(6, np.float64, (Q, G, T))
            sec_in, eps_in, mode_in, near_in = view(7, np.int32, (Q,)), view(8, np.float64, (Q,)), view(9, np.int32, (Q,)), view(10, np.float64, (Q,))
            u_in, ur_in = view(11, np.int64, (Q,)), view(12, row_t, (total_u * width,))
            at = at_y = at_u = 0
            for i in order:
                q = queries[i]
                w_in[q, :, :self.S], th_in[q], b_in[q], l_in[q] = wg[i], th[i], float(ballasts[i]), counts[i]
                r_in[at:at + rs[i].size], y_in[at_y:at_y + ys[i].size] = rs[i], ys[i]
                at += rs[i].size
                at_y += ys[i].size
                sec_in[q], eps_in[q] = int(seconds[i]), eps[i]
                mode_in[q], near_in[q] = (1, 0.0) if reaches[i] is None else (0, float(reaches[i]))
                u_in[q] = us[i].size // width
                ur_in[at_u:at_u + us[i].size] = us[i]
                at_u += us[i].size
                if given:
                    surface[q] = sf[i]
            last = getattr(self, "_bround_last", None)
            if last is None or max(queries) >= last[0]:
                # no batched round, or a query it did not have: VQ_E_STATE as the library gives it, also for an entry without labels
                # (a slot the library would skip) -- there is no block of that round to hand it
                raise _lib.VqError(-4, "no batched round has run on this handle" if last is None else
                                   "the last batched round had %d queries (asked for %r)" % (last[0], queries))
            _Q, roff, start, pool, sims = last
            blk = self._batch_round_block(_Q)[0] if pool is None else self._pooled_block("_view_round_pools", roff[9])
            rview = self._block_view(blk.bytes(), roff)
            call("vq_db_batch_round_update_given" if tables else "vq_db_batch_round_update", self._h, Q, G, T, total, total_u, C.c_void_p(ublk.ptr),
                 ublk.nbytes, C.c_void_p(blk.ptr), blk.nbytes, flags)
            pick, idx = view(13, np.float64, (Q, 8)), view(14, np.int32, (Q, 4))
            decode = self._partition_decoder(rview, roff, _Q)
            out = []
            for i, q in enumerate(queries):
                r = UpdateResult()
                served = counts[i] > 0                        # a slot without labels is skipped: it stays what the round left
                r.avg, r.n_e = sims[q]
                r.scores = rview(5, np.float64, (start[q + 1] - start[q],), start[q]) if want_scores and served else None
                decode(r, q, served)
                r.surface = surface[q] if want_surface and served else None
                if served:
                    r.w, r.threshold, r.lowest, r.band = pick[q, 0], pick[q, 1], pick[q, 2], (float(pick[q, 3]), float(pick[q, 4]))
                    r.iw, r.it, r.on_rim, r.fell_back = int(idx[q, 0]), int(idx[q, 1]), bool(idx[q, 2] & 1), bool(idx[q, 2] & 2)
                else:
                    r.w = r.threshold = r.lowest = r.band = r.iw = r.it = r.on_rim = r.fell_back = None
                out.append(r)
            return out

    # ------------------------------------------------------------------ the k best clips of every query of a batched round
    def batch_topk_cap(self) -> int:
        """The largest k :meth:`batch_round_topk` ranks (the library's constant, read through vq_db_batch_topk_layout)."""
        off = (C.c_int64 * 6)()
        call("vq_db_batch_topk_layout", self._h, 1, 1, off)
        return int(off[5])

    def batch_round_topk(self, ks, queries=None) -> list:
        """ticket.py:266 for several queries of the LAST batched round (either kind, whether or not it copied its scores back) in ONE
        call (vq_db_batch_round_topk, include/vq_amd_round_topk.h): the ``ks[i]`` best clips of query ``queries[i]`` of that round
        (``queries`` None: all of them, in order; ``ks`` an int: the same k for each), ranked on the device from the scores the
        round -- or a :meth:`batch_round_rescore` behind it -- left there.  One (rows, vals) per entry, as :meth:`topk` gives them:
        positions in the query's view (as in every result of that round) by descending score, ties by ascending position, NaN
        excluded, and the scores at those positions bit for bit.  A k above the rows of the query's view is clamped to them; one
        above :meth:`batch_topk_cap` is the library's refusal.  Without a batched round: ``VqError`` (VQ_E_STATE)."""
        with self.lock:
            last = getattr(self, "_bround_last", None)
            if queries is None:
                queries = list(range(last[0])) if last is not None else [0]
            queries = [int(q) for q in queries]
            n = len(queries)
            kk = [int(ks)] * n if np.ndim(ks) == 0 else [int(v) for v in ks]
            if not n or len(kk) != n or len(set(queries)) != n or min(queries) < 0 or max(queries) >= 16:
                raise ValueError("one k per query (or one int), every query -- its index in the last batched round -- once")
            if min(kk) < 0:
                raise ValueError("k must not be negative")
            if last is not None:                              # min(k, M_q); a query the round did not have keeps its k: the library refuses it
                start = last[2]
                kk = [min(k, start[q + 1] - start[q]) if q < last[0] else max(k, 1) for k, q in zip(kk, queries)]
            Q, k_max = max(queries) + 1, max(max(kk), 1)
            off = (C.c_int64 * 6)()
            call("vq_db_batch_topk_layout", self._h, Q, k_max, off)
            off = [int(v) for v in off]
            blk = self._pooled_block("_topk_pools", off[4])
            view = self._block_view(blk.bytes(), off)
            k_in, count = view(0, np.int64, (Q,)), view(1, np.int64, (Q,))
            k_in[...] = 0
            count[...] = 0
            for q, k in zip(queries, kk):
                k_in[q] = k
            call("vq_db_batch_round_topk", self._h, Q, k_max, C.c_void_p(blk.ptr), blk.nbytes)
            rows, vals = view(2, np.int64, (Q, k_max)), view(3, np.float64, (Q, k_max))
            return [(rows[q, :int(count[q])], vals[q, :int(count[q])]) for q in queries]

    def rescore(self, weights: Sequence[float]):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (self.S,):
            raise ValueError("one weight per stream")
        with self.lock:
            call("vq_db_rescore", self._h, _np_ptr(w))

    def similarities(self, sims: bool = False):
        avg = np.empty((self._na, self.S), dtype=np.float64)
        ne = np.empty((self._na, self.S), dtype=np.int32)
        sm = np.empty((self._na, self.S, self.E), dtype=np.float64) if sims else None
        call("vq_db_read_similarities", self._h, _np_ptr(avg), _np_ptr(ne), _np_ptr(sm) if sims else None)
        return (avg, ne, sm) if sims else (avg, ne)

    def write_avg(self, avg: np.ndarray, n_e: np.ndarray | None = None):
        a = np.ascontiguousarray(avg, dtype=np.float64)
        ne = None if n_e is None else np.ascontiguousarray(n_e, dtype=np.int32)
        with self.lock:
            if a.size != self._na * self.S or (ne is not None and ne.size != a.size):
                raise ValueError("avg / n_e must be [%d,%d]: what the database (or the search set in use) covers" % (self._na, self.S))
            call("vq_db_write_avg", self._h, _np_ptr(a), _np_ptr(ne) if ne is not None else None)

    def scores(self) -> np.ndarray:
        out = np.empty(self._na, dtype=np.float64)
        call("vq_db_read_scores", self._h, _np_ptr(out))
        return out

    def scores_grid(self, w_grid: np.ndarray, rows: Sequence[int]) -> np.ndarray:
        wg = np.ascontiguousarray(w_grid, dtype=np.float64)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if wg.ndim != 2 or wg.shape[1] != self.S:
            raise ValueError("w_grid must be [G,%d]" % self.S)
        out = np.empty((wg.shape[0], r.shape[0]), dtype=np.float64)
        call("vq_db_scores_grid", self._h, _np_ptr(wg), wg.shape[0], _np_ptr(r), r.shape[0], _np_ptr(out))
        return out

    def loss_surface(self, w_grid: np.ndarray, rows: Sequence[int], labels: Sequence[float], th_grid: np.ndarray, ballast: float) -> np.ndarray:
        """hyperparameter.py:57-64 in one launch: [G, T] sums of the loss over the labelled rows (in order) for every grid weight and
        grid threshold, starting from 0.5 * threshold; the caller divides by the number of labels (include/vq_amd.h)."""
        wg = np.ascontiguousarray(w_grid, dtype=np.float64)
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        y = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1)
        th = np.ascontiguousarray(th_grid, dtype=np.float64).reshape(-1)
        if wg.ndim != 2 or wg.shape[1] != self.S or y.shape != r.shape:
            raise ValueError("w_grid must be [G,%d] and one label per row" % self.S)
        out = np.empty((wg.shape[0], th.size), dtype=np.float64)
        call("vq_db_loss_surface", self._h, _np_ptr(wg), wg.shape[0], _np_ptr(r), _np_ptr(y), r.size, _np_ptr(th), th.size, float(ballast), _np_ptr(out))
        return out

    def select(self, threshold: float, lower: float):
        """Order-preserving partition (ticket.py:325-340): (match_rows, near_rows, near_argmax).  Partition and
        copy-out are one locked call of the library, so handles shared between broker threads stay consistent; ``self.lock`` keeps
        it out of another thread's :meth:`query_round`, whose lists it would replace."""
        nm, nn, am = C.c_int64(), C.c_int64(), C.c_int64()
        with self.lock:
            m = np.empty(max(self._na, 1), dtype=np.int64)
            r = np.empty(max(self._na, 1), dtype=np.int64)
            call("vq_db_select_rows", self._h, float(threshold), float(lower), _np_ptr(m), m.size, _np_ptr(r), r.size,
                 C.byref(nm), C.byref(nn), C.byref(am))
        return m[:nm.value].copy(), r[:nn.value].copy(), am.value

    def topk(self, k: int):
        with self.lock:                                       # the radix form reuses (and invalidates) the selection lists of the handle
            k = int(min(k, self._na))
            if k <= 0 and self._na == 0:                      # an empty search set has no best clips
                return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64)
            rows = np.empty(k, dtype=np.int64)
            vals = np.empty(k, dtype=np.float64)
            kk = C.c_int64()
            call("vq_db_topk", self._h, k, _np_ptr(rows), _np_ptr(vals), C.byref(kk))
        return rows[:kk.value], vals[:kk.value]

    def min_score(self, rows: Sequence[int]) -> float:
        r = np.ascontiguousarray(rows, dtype=np.int64)
        out = C.c_double()
        call("vq_db_min_score", self._h, _np_ptr(r) if r.size else None, r.size, C.byref(out))
        return out.value

    # ------------------------------------------------------------------ index
    def row_of(self, clip_id: int) -> int:
        if self._row_of is None:
            self._row_of = {int(c): i for i, c in enumerate(self.clip_ids.tolist())}
        return self._row_of[int(clip_id)]

    def has_clip(self, clip_id) -> bool:
        if self._row_of is None:
            self.row_of(int(self.clip_ids[0]))
        try:
            return int(clip_id) in self._row_of
        except (TypeError, ValueError):
            return False

    def close(self):
        if self._h:
            pools = [getattr(self, "_round_pool", None)] + [p for _off, p in getattr(self, "_batch_round_pools", {}).values()] + \
                list(getattr(self, "_view_round_pools", {}).values()) + list(getattr(self, "_fit_pools", {}).values()) + \
                list(getattr(self, "_topk_pools", {}).values()) + list(getattr(self, "_grid_pools", {}).values()) + \
                list(getattr(self, "_update_pools", {}).values()) + list(getattr(self, "_target_pools", {}).values())
            self._bround_last = None
            for pool in pools:
                if pool is None:
                    continue
                pool["closed"] = True                         # blocks still referenced by result arrays free themselves
                while pool["free"]:
                    _lib.load().vq_host_free(C.c_void_p(pool["free"].pop()[0]))
            _lib.load().vq_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
