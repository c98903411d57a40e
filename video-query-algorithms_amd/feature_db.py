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
from .batch_rounds import ONE_ROUND, BatchRounds, RoundResult, UpdateResult, _np_ptr          # noqa: F401 (the results: importable from here)
from .host_blocks import BlockRegistry, _RoundBlock                                           # noqa: F401

_VQ_DTYPE = {np.dtype(np.float16): VQ_F16, np.dtype(np.float32): VQ_F32, np.dtype(np.float64): VQ_F64}


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


# the layouts of vq_db_set_layout by name (include/vq_amd.h); the values also travel as they are in ShardedFeatureDB's OP_LAYOUT
_LAYOUTS = {"rows": _lib.VQ_LAYOUT_ROWS, "tiled": _lib.VQ_LAYOUT_TILED, "tiled64": _lib.VQ_LAYOUT_TILED64}
_LAYOUT_NAMES = {v: k for k, v in _LAYOUTS.items()}
# The public table: every layout by name.  _LAYOUTS above stays the three names it held when "tiled64" was the last one, because
# tests/test_tiled64_host.py holds it (and sharded_db.LAYOUT_VALUES) to exactly those; set_layout, layout, from_csv_tree and both ends of
# ShardedFeatureDB's OP_LAYOUT look names up HERE.
LAYOUTS = dict(_LAYOUTS, tiled16=_lib.VQ_LAYOUT_TILED16)
LAYOUT_NAMES = {v: k for k, v in LAYOUTS.items()}
_TILED_OF_DTYPE = {np.dtype(np.float32): "tiled", np.dtype(np.float64): "tiled64", np.dtype(np.float16): "tiled16"}

def _pad_for(dim):
    """What the constructors that take data of any length pass as ``short_rows``: True for a length that is no multiple of 4 (stored
    padded, short rows on their own kernel), None for any other (the plain database of ever)."""
    return True if dim is not None and int(dim) % 4 != 0 else None


def whole_view(db) -> SearchSetView:
    """The trivial view of a database object (FeatureDB, ShardedFeatureDB, or a look-alike with ``clip_ids`` and ``row_of``)."""
    n = len(db.clip_ids)
    return SearchSetView(None, db.clip_ids, np.arange(n, dtype=np.int64), whole=db)


def search_set_rows(db, clip_ids) -> np.ndarray:
    """Clip ids -> the strictly ascending database rows of a search set (duplicates collapse; an unknown id is a KeyError)."""
    return np.unique(np.fromiter((db.row_of(c) for c in clip_ids), dtype=np.int64))


class FeatureDB(BatchRounds):
    """N clips x S streams x E ensemble slots x D floats, resident on ``device``.  ``dtype`` is how the block is STORED: float32, float64
    or (opt-in) float16 -- half the bytes per query and per clip; values are rounded once on the way in and every result is what the
    fp64 arithmetic gives on the rounded values.

    ``dim`` is any length >= 1 (the 101 class scores of ``fc-action`` as well as 1024 pooled activations).  ``D`` is that logical length,
    what every array the caller hands in or gets back has; ``Dp`` is the stored pitch, ``D`` rounded up to a multiple of 4, with
    +0.0 pads that the methods below write on the way in and cut on the way out (include/vq_amd_dim.h).  The plain constructor keeps
    what it ever did -- ``vq_db_create`` as it was, a ``dim`` that is no multiple of 4 is a ``VqError`` -- and padding is asked for:
    ``short_rows=True`` makes the handle with ``VQ_DIM_PADDED | VQ_DIM_SHORT_ROWS`` (stored ``Dp <= 128`` then scans with the short-row
    kernel), ``short_rows=False`` with ``VQ_DIM_PADDED`` alone when ``dim % 4 != 0`` (the generic kernel) and plainly otherwise.
    ``from_arrays``, ``from_records``, ``from_store`` and ``from_csv_tree`` ask for ``short_rows=True`` whenever their data's length is no
    multiple of 4.  Out of scope on a padded database (``D != Dp``): ``scan_batch``, the batched rounds, ``synthetic``."""

    def __init__(self, n: int, n_streams: int, n_splits: int, dim: int = 1024, dtype=np.float32, device: int = 0,
                 clip_ids: Sequence[int] | None = None, short_rows: bool | None = None):
        # before anything can fail, so that close() always finds them: the handle, and the pools of page-locked blocks of every
        # call that takes one -- made here, not on first use, so that the first calls of two threads share them
        self._h = C.c_void_p()
        self.blocks = BlockRegistry()
        BatchRounds.__init__(self)
        self.n, self.S, self.E, self.D = int(n), int(n_streams), int(n_splits), int(dim)
        self.dtype = np.dtype(dtype)
        if self.dtype not in _VQ_DTYPE:
            raise TypeError("FeatureDB dtype must be float32, float64 or float16")
        self.device = int(device)
        self.Dp = (self.D + 3) // 4 * 4
        flags = 0
        if short_rows:
            flags = _lib.VQ_DIM_PADDED | _lib.VQ_DIM_SHORT_ROWS
        elif short_rows is False and self.D % 4 != 0:
            flags = _lib.VQ_DIM_PADDED
        call("vq_db_create", self.n, self.S, self.E, self.D, _VQ_DTYPE[self.dtype] | flags, self.device, C.byref(self._h))
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
        self._round_off = self._layout(ONE_ROUND, "vq_db_round_layout")

    # ------------------------------------------------------------------ logical length and stored pitch
    def _padded(self, t: np.ndarray) -> np.ndarray:
        """[..., D] float64 -> the contiguous [..., Dp] block the library takes, +0.0 in the pads (the array itself when D == Dp)."""
        if self.D == self.Dp:
            return t
        out = np.zeros(t.shape[:-1] + (self.Dp,), dtype=np.float64)
        out[..., :self.D] = t
        return out

    def _logical(self, a: np.ndarray) -> np.ndarray:
        """[..., Dp] as the library wrote it -> [..., D], contiguous."""
        return a if self.D == self.Dp else np.ascontiguousarray(a[..., :self.D])

    def _layout(self, pieces: dict, name: str, *args):
        # every batched call lays its block out first: a padded database takes one-query rounds only (include/vq_amd_dim.h)
        if self.D != self.Dp and name != "vq_db_round_layout":
            raise ValueError("batched rounds are out of scope for a database of length %d stored at pitch %d" % (self.D, self.Dp))
        return BatchRounds._layout(self, pieces, name, *args)

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
        db = cls(n, s, e, d, feats.dtype if dtype is None else dtype, device, clip_ids, short_rows=_pad_for(d))
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
                 np.fromiter(order.keys(), dtype=np.int64, count=n), short_rows=_pad_for(dim))
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
        db = cls(rows, feats.shape[1], feats.shape[2], feats.shape[3], feats.dtype, device, ids[row0:row0 + rows], short_rows=_pad_for(feats.shape[3]))
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
        ``(video, clip)`` of every row; ``csv_host_fields`` counts the fields the host had to resolve.  ``layout="tiled"`` (fp32), ``"tiled64"`` (fp64) or ``"tiled16"`` (fp16) tiles the
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
        db = cls(n, len(streams), len(splits), dim, dtype, device, clip_id_base + np.arange(1, n + 1, dtype=np.int64), short_rows=_pad_for(dim))
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
        """Rows generated on the device by the counter-based hash (oracle.sim_oracle.synth_features); ``dim`` a multiple of 4 (the
        generator fills whole stored vectors)."""
        if int(dim) % 4 != 0:
            raise ValueError("synthetic rows need dim % 4 == 0 (got %d)" % dim)
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
        # D != Dp: the library takes the unpadded rows and writes them at pitch with zero pads on the device (include/vq_amd_dim.h)
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
        """"rows" ([N][S][E][D]), "tiled" ([tile of 16 clips][S*E][D/4][clip][4]: the order in which every load of the scans
        takes whole lines; float32 only), "tiled64" (the same for float64: [tile][S*E][D/2][clip][2]) or "tiled16" (for float16:
        [tile][S*E][D/8][clip][8]); all need D = 1024, S <= 2, E <= 5 and each is refused for the others' dtypes (:attr:`layouts`
        names what this database takes).  In place, one sweep of the block: call once after loading.  Never chosen for the caller:
        the layouts agree to rounding, not bit for bit.  A name that is no layout is a ``KeyError``."""
        call("vq_db_set_layout", self._h, LAYOUTS[layout])      # LAYOUTS, not _LAYOUTS: see the comment at the tables

    @property
    def layout(self) -> str:
        v = C.c_int32()
        call("vq_db_layout", self._h, C.byref(v))
        return LAYOUT_NAMES[v.value]

    @property
    def layouts(self) -> tuple:
        """The names :meth:`set_layout` accepts for this database, "rows" first: ``("rows", "tiled16")`` for a float16 database of
        a tileable shape, ``("rows", "tiled")`` / ``("rows", "tiled64")`` for float32 / float64, ``("rows",)`` for any other shape.
        By dtype and shape alone: a block that is not the library's alone any more (adopted, or its address handed out) is refused
        whatever the name (``VqError``, VQ_E_STATE)."""
        if not (self.Dp == 1024 and 1 <= self.S <= 2 and 1 <= self.E <= 5):      # the stored pitch: D = 1021 .. 1024
            return ("rows",)
        return ("rows", _TILED_OF_DTYPE[np.dtype(self.dtype)])

    @property
    def tiled_layout(self):
        """The float32 / float64 name: "tiled" (float32), "tiled64" (float64), or ``None`` (a shape without the tiled kernels -- and
        float16, whose "tiled16" came later: this property keeps the value it had for every database, tests/test_tiled64_gpu.py holds
        it to ``None`` there).  :attr:`layouts` is the way to ask what a database takes, whichever its dtype."""
        if self.dtype == np.float16 or not (self.Dp == 1024 and 1 <= self.S <= 2 and 1 <= self.E <= 5):
            return None
        return "tiled64" if self.dtype == np.float64 else "tiled"

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
        out = np.empty((r.size, self.S, self.E, self.Dp), dtype=self.dtype)
        call("vq_db_read_rows", self._h, _np_ptr(r) if r.size else None, int(r.size), _np_ptr(out))
        return self._logical(out)

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
        t = self._padded(t)
        with self.lock:
            call("vq_db_set_query", self._h, _np_ptr(t))

    def set_query_from_row(self, row: int, want: bool = True):
        """t = r/(r.r) of a resident row (target_clip.py:311-313), computed on the device."""
        out = np.empty((self.S, self.E, self.Dp), dtype=np.float64) if want else None
        with self.lock:
            call("vq_db_set_query_from_row", self._h, int(row), _np_ptr(out) if want else None)
        return self._logical(out) if want else None

    def bootstrap_target(self, valid_rows: Sequence[int], invalid_rows: Sequence[int] = (), mu: float = 0.0,
                         set_query: bool = True) -> np.ndarray:
        """New query vectors [S,E,D] from user-validated resident clips (target_clip.py:161-261, closed forms on the
        device; see csrc/vq_boot.hip).  With ``set_query`` they become the query of the next scan."""
        v = np.ascontiguousarray(valid_rows, dtype=np.int64)
        iv = np.ascontiguousarray(invalid_rows, dtype=np.int64)
        out = np.empty((self.S, self.E, self.Dp), dtype=np.float64)
        with self.lock:
            call("vq_db_bootstrap_target", self._h, _np_ptr(v), int(v.size), _np_ptr(iv) if iv.size else None, int(iv.size), float(mu),
                 _np_ptr(out), 1 if set_query else 0)
        return self._logical(out)

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
        if self.D != self.Dp:
            raise ValueError("scan_batch is out of scope for a database of length %d stored at pitch %d" % (self.D, self.Dp))
        out = np.empty((t.shape[0], self.n), dtype=np.float64) if want else None
        call("vq_db_scan_batch", self._h, t.shape[0], _np_ptr(t), _np_ptr(w), _np_ptr(out) if want else None)
        return out

    # ------------------------------------------------------------------ a query round in one call
    def query_round(self, t: np.ndarray | None, weights=None, select=None) -> RoundResult:
        """ticket.py:120-180,311-356 as ONE call of the library (vq_db_query_round): one lock, one synchronisation, one copy back.
        ``t`` [S,E,D]: scan under this query (None: the similarities the handle holds); ``weights`` [S]: scores under them;
        ``select`` = (threshold, lower): the order-preserving partition.  Bit for bit what set_query / scan / similarities / rescore /
        scores / select return one by one (tested); the arrays are views of page-locked memory that stay valid as long as they live.
        The round and the fetch of a list longer than its 1024-row prefix run under ``self.lock``, which every method that replaces
        the handle's scores or selection lists takes: the lists are this round's whatever other threads ask of the handle."""
        off = self._round_off
        blk = self.blocks.take("round", off["bytes"])        # before the lock: the registry has its own
        view = self._block_view(blk.bytes(), off)
        S = self.S
        flags = 0
        if t is not None:
            tv = view("t", np.float64, (S, self.E, self.Dp))
            tv[..., :self.D] = t
            if self.D != self.Dp:
                tv[..., self.D:] = 0.0                        # the block is reused: the pads are written every time
            flags |= 1
        if weights is not None:
            view("weights", np.float64, (S,))[...] = weights
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
            r.avg = view("avg", np.float64, (n, S)) if t is not None else None
            r.n_e = view("n_e", np.int32, (n, S)) if t is not None else None
            r.scores = view("scores", np.float64, (n,)) if weights is not None else None
            r.match_rows = r.near_rows = None
            r.near_argmax = -1
            if select is not None:
                res = view("result", np.int64, (4,))
                nm, nn, r.near_argmax = int(res[0]), int(res[1]), int(res[2])
                if nm <= off["prefix"] and nn <= off["prefix"]:
                    r.match_rows = view("match_prefix", np.int64, (nm,))
                    r.near_rows = view("near_prefix", np.int64, (nn,))
                else:                                         # a list longer than its prefix: the full lists are still on the device
                    m = np.empty(nm, dtype=np.int64)
                    q = np.empty(nn, dtype=np.int64)
                    call("vq_db_select_fetch", self._h, _np_ptr(m) if nm else None, nm, _np_ptr(q) if nn else None, nn)
                    r.match_rows, r.near_rows = m, q
        return r

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
            self._bround_last = None
            self.blocks.close()                               # blocks still referenced by result arrays free themselves
            _lib.load().vq_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
