"""Batched query rounds on one handle: up to 16 rounds in one pass over the database and the calls on what such a round leaves on
the device -- weight fits, re-weighting, the one-call update, the k best clips, the bootstrapped targets.  The host side of
include/vq_amd_round*.h: :class:`BatchRounds` is the base of :class:`feature_db.FeatureDB` that carries these methods; the layout
tables below name the pieces of every block in the order its header documents."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import call


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _pieces(names: str) -> dict:
    return {name: i for i, name in enumerate(names.split())}


# piece name -> index into the offsets of a layout call; "bytes" is the length of the block, what follows it are the call's constants
ONE_ROUND = _pieces("t weights avg n_e scores result match_prefix near_prefix bytes prefix")                     # vq_amd.h
ROUND = _pieces("t weights band n_e avg scores result match_prefix near_prefix bytes prefix sum_m")              # vq_amd_rounds.h, _round_views.h
_FIT_INPUTS = "w_grid th_grid ballast L rows labels surface "
FIT = _pieces(_FIT_INPUTS + "bytes")                                                                             # vq_amd_round_fit.h
UPDATE = _pieces(_FIT_INPUTS + "second eps band_mode near U user_rows pick pick_idx bytes")                      # vq_amd_round_update.h
GRID = _pieces("w_grid L rows graded bytes")                                                                     # vq_amd_round_grid.h
AVG_ROWS = _pieces("L rows avg_rows bytes")                                                                      # vq_amd_round_shard.h
TOPK = _pieces("k count rows vals bytes cap")                                                                    # vq_amd_round_topk.h
TARGETS = _pieces("query param rows draw pos work previous status target bytes lds_rows")                        # vq_amd_round_targets.h


class Layout(list):
    """The byte offsets a layout call gave, numbered as in its header and addressed by piece name (``pieces``: one of the tables above; ``at``: name -> offset)."""

    def __init__(self, pieces: dict, off):
        super().__init__(int(v) for v in off)
        self.at = dict(zip(pieces, self))

    def __getitem__(self, piece):
        return self.at[piece] if isinstance(piece, str) else super().__getitem__(piece)


class RoundResult:
    """What one call of :meth:`FeatureDB.query_round` brought back (numpy views of one page-locked block)."""
    __slots__ = ("avg", "n_e", "scores", "match_rows", "near_rows", "near_argmax")


class UpdateResult(RoundResult):
    """What :meth:`FeatureDB.batch_round_update` brought back for one query: the fields of the rescore's :class:`RoundResult` and the
    pick -- ``w`` (the fitted grid weight), ``threshold``, ``lowest`` (the lowest-scoring confirmed match of a finalize member, else
    1.0), ``band`` = (threshold, lower), ``iw`` / ``it`` (the cell), ``on_rim``, ``fell_back``, and ``surface`` [G,T] when asked."""
    __slots__ = ("w", "threshold", "lowest", "band", "iw", "it", "on_rim", "fell_back", "surface")


@dataclass(frozen=True)
class LastRound:
    """The last batched round of a handle: what the calls on it lay their block out by, and the round's avg / n_e their results carry."""
    Q: int              # its number of queries
    off: Layout         # the layout of its block (ROUND)
    start: list         # [Q + 1]: query q's results are elements [start[q], start[q + 1]) of the per-row pieces
    views: bool         # a search set per query (query_round_batch_sets), or the whole database
    sims: list          # (avg, n_e) of every query, as the round returned them

    def block(self, blocks):
        """A block for a call on this round, laid out like the round's own, from the pool that one came from."""
        return blocks.take("view_round" if self.views else "batch_round", self.off["bytes"])

    def rows(self, q: int) -> int:
        return self.start[q + 1] - self.start[q]


def entry_arrays(S: int, queries, rows=None, labels=None, w_grids=None, th_grids=None, others=(), row_t=np.int64, width: int = 1):
    """The per-entry arguments of a batched call as arrays, checked: (queries, rows, labels, w_grids, th_grids, G, T), None (and G, T
    = 0) for what the call does not take.  One of each argument (``others``: those that only count) per query and every query
    once; w_grids [G,S] and th_grids [T] with one G and one T for the call; one label per row of ``width`` elements."""
    queries = [int(q) for q in queries]
    k = len(queries)
    if not k or any(a is not None and len(a) != k for a in (rows, labels, w_grids, th_grids) + tuple(others)) or len(set(queries)) != k:
        raise ValueError("one rows / labels / w_grid / th_grid (and every other per-entry argument) per query, every query once")
    wg = None if w_grids is None else [np.asarray(w, dtype=np.float64) for w in w_grids]
    th = None if th_grids is None else [np.asarray(t, dtype=np.float64).reshape(-1) for t in th_grids]
    rs = None if rows is None else [np.asarray(r, dtype=row_t).reshape(-1) for r in rows]
    ys = None if labels is None else [np.asarray(y, dtype=np.float64).reshape(-1) for y in labels]
    G = 0 if wg is None else int(wg[0].shape[0]) if wg[0].ndim == 2 else -1
    T = 0 if th is None else int(th[0].size)
    if any(w.ndim != 2 or w.shape != (G, S) for w in wg or ()) or any(t.size != T for t in th or ()) or \
            (ys is not None and any(r.size != y.size * width for r, y in zip(rs, ys))):
        raise ValueError("w_grids must be [G,%d] and th_grids [T] with one G and T for the call, and one label per row%s"
                         % (S, " of [., %d] averaged similarities" % S if width > 1 else ""))
    if min(queries) < 0:
        raise ValueError("a query is its index in the last batched round")
    return queries, rs, ys, wg, th, G, T


def pack_slots(view, Q: int, queries, slots=(), lists=()):
    """Fill the slot-ordered inputs of a block of ``Q`` slots, slot q = query q of the round.  ``slots``: (piece, dtype, shape of a
    slot, one value per entry) -- the piece [Q, *shape] is zeroed, then entry i's value goes to the front of slot ``queries[i]`` (a
    row of weights is padded that way).  ``lists``: (piece, dtype, width, one flat array per entry) -- concatenated in ascending
    slot order.  Returns, per list, every entry's first element in units of ``width``: where its share of an output starts."""
    for piece, dtype, shape, values in slots:
        arr = view(piece, dtype, (Q,) + shape)
        arr[...] = 0
        if len(values):                                       # all entries in one assignment: the queries are distinct
            used = np.asarray(values, dtype=dtype)            # a value the piece's type cannot hold is an error here, not a wrap
            arr[(list(queries),) + tuple(slice(n) for n in used.shape[1:])] = used
    order = sorted(range(len(queries)), key=queries.__getitem__)
    firsts = []
    for piece, dtype, width, arrays in lists:
        flat = view(piece, dtype, (sum(a.size for a in arrays),))
        at, first = 0, [0] * len(arrays)
        for i in order:
            flat[at:at + arrays[i].size] = arrays[i]
            first[i] = at // width
            at += arrays[i].size
        firsts.append(first)
    return firsts


class BatchRounds:
    """The batched-round methods of a database handle.  The handle provides ``_h``, ``lock``, ``blocks`` (its BlockRegistry), n, S, E,
    D and the search sets (``_sets``, ``has_search_set``)."""

    def __init__(self):
        self._bround_last = None                              # the LastRound the calls on a round work on
        self._bround_layouts = {}                             # Q -> the layout of a whole-database round (it depends on Q alone)

    def _layout(self, pieces: dict, name: str, *args) -> Layout:
        """The offsets the layout call ``name`` gives for ``args``, by piece."""
        off = (C.c_int64 * len(pieces))()
        call(name, self._h, *args, off)
        return Layout(pieces, off)

    def _slot_block(self, kind: str, pieces: dict, layout: str, queries, *dims):
        """(Q, block, view) for a call whose block has a slot per query of the last round up to the largest of ``queries`` -- slot q =
        query q; the library refuses what that round lacks -- laid out by the call ``layout`` for (Q, *dims)."""
        Q = max(queries) + 1
        off = self._layout(pieces, layout, Q, *dims)
        blk = self.blocks.take(kind, off["bytes"])
        return Q, blk, self._block_view(blk.bytes(), off)

    # ------------------------------------------------------------------ up to 16 query rounds in one pass
    def batch_round_supported(self) -> bool:
        """Does this database meet the preconditions of the 16-query pass (include/vq_amd_rounds.h)?  The whole database only: the
        caller selects it first (``use_search_set(None)``)."""
        return self.D in (256, 512, 768, 1024) and self.S <= 8

    @staticmethod
    def _block_view(raw: np.ndarray, off: Layout):
        """view(piece, dtype, shape, first=0) over a block laid out by ``off`` (kept as ``view.off``): ``shape`` elements of ``piece``,
        from its element ``first`` on -- one array over ``raw``'s memory (its ``.base``); one that would pass the block's end is an error."""
        at = off.at

        def view(piece, dtype, shape, first=0):
            return np.ndarray(shape, dtype, raw, at[piece] + first * np.dtype(dtype).itemsize)
        view.off = off
        return view

    def _fill_round_inputs(self, view, Q: int, slots, w, bands, t=None) -> int:
        """The inputs of a batched round's block of ``Q`` queries: the targets (a round), and for the queries ``slots`` their weights
        (padded to 8) and bands; ``slots`` indexes the rows of [Q, ...] arrays.  Returns the partition flag the bands ask for."""
        if t is not None:
            view("t", np.float64, (Q, self.S, self.E, self.D))[...] = t
        wv, bv = view("weights", np.float64, (Q, 8)), view("band", np.float64, (Q, 2))
        wv[...] = 0.0
        bv[...] = 0.0
        wv[slots, :self.S] = w
        if bands is None:
            return 0
        bv[slots] = bands
        return _lib.VQ_BROUND_SELECT

    def _partition_decoder(self, view, off: Layout, Q: int):
        """decode(r, q, have): the partition of query q of the last batched round into ``r`` from the block's results and prefixes;
        a list longer than its prefix is fetched (the full lists are still on the device).  Call under ``self.lock``."""
        res = view("result", np.int64, (Q, 4))
        prefix = off["prefix"]
        pre_m, pre_n = view("match_prefix", np.int64, (Q, prefix)), view("near_prefix", np.int64, (Q, prefix))

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

    def _whole_round_plan(self, Q: int):
        """(layout, start, kind of block, library call, its arguments in front of the block) of a round over the whole database;
        the layout depends on Q alone and is kept.  Q outside [1, 16]: the library's own refusal (VqError)."""
        if Q not in self._bround_layouts:
            self._bround_layouts[Q] = self._layout(ROUND, "vq_db_batch_round_layout", Q)
        return self._bround_layouts[Q], [q * self.n for q in range(Q + 1)], "batch_round", "vq_db_query_round_batch", (Q,)

    def _view_round_plan(self, Q: int, set_ids):
        """The same for a round with a search set per query: the layout depends on the sets, so its blocks are pooled by size."""
        tokens = (C.c_int32 * max(Q, 1))()
        for q, sid in enumerate(set_ids):
            if sid is not None and not self.has_search_set(sid):
                raise _lib.VqError(-1, "query %d: search set %r is not defined on this database" % (q, sid))
            tokens[q] = -1 if sid is None else self._sets[sid].token
        off, start = (C.c_int64 * len(ROUND))(), (C.c_int64 * 17)()
        call("vq_db_view_round_layout", self._h, Q, tokens, off, start)                  # Q outside [1, 16]: the library's own refusal
        return Layout(ROUND, off), [int(v) for v in start], "view_round", "vq_db_query_round_views", (Q, tokens)

    def _batch_round(self, targets, weights, selects, want_avg, timed, want_scores, set_ids=None) -> list:
        """The two rounds: over the whole database (``set_ids`` None: ONE n_e array shared by all results) or a search set per query."""
        t = np.asarray(targets, dtype=np.float64)
        w = np.asarray(weights, dtype=np.float64)
        if t.ndim != 4 or t.shape[1:] != (self.S, self.E, self.D) or w.shape != (t.shape[0], self.S):
            raise ValueError("targets must be [Q,%d,%d,%d] and weights [Q,%d]" % (self.S, self.E, self.D, self.S))
        Q, S, whole = int(t.shape[0]), self.S, set_ids is None
        if not whole:
            set_ids = list(set_ids)
            if len(set_ids) != Q:
                raise ValueError("one search set id (or None) per query")
        bands = None if selects is None else np.asarray(selects, dtype=np.float64)
        if bands is not None and bands.shape != (Q, 2):
            raise ValueError("selects must be [Q,2]: (threshold, lower) per query")
        with self.lock:
            plan = self._whole_round_plan(Q) if whole else None        # refused (Q outside [1, 16]): the round before stays
            self._bround_last = None                          # the round before is gone (its block may serve this one)
            off, start, kind, name, args = plan or self._view_round_plan(Q, set_ids)
            blk = self.blocks.take(kind, off["bytes"])
            view = self._block_view(blk.bytes(), off)
            flags = (_lib.VQ_BROUND_SCORES if want_scores else 0) | (_lib.VQ_BROUND_AVG if want_avg else 0) | (_lib.VQ_BROUND_TIMED if timed else 0)
            flags |= self._fill_round_inputs(view, Q, slice(None), w, bands, t)
            call(name, self._h, *args, C.c_void_p(blk.ptr), blk.nbytes, flags)
            decode = self._partition_decoder(view, off, Q)
            n_e = view("n_e", np.int32, (self.n, S)) if whole and want_avg else None
            out = []
            for q in range(Q):
                m, at = start[q + 1] - start[q], start[q]
                r = RoundResult()
                r.avg = view("avg", np.float64, (m, S), at * S) if want_avg else None
                r.n_e = n_e if whole or not want_avg else view("n_e", np.int32, (m, S), at * S)
                r.scores = view("scores", np.float64, (m,), at) if want_scores else None
                decode(r, q, bands is not None)
                out.append(r)
            # what the calls on this round lay their block out by, and the round's avg / n_e their results carry
            self._bround_last = LastRound(Q, off, start, not whole, [(r.avg, r.n_e) for r in out])
            return out

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
        return self._batch_round(targets, weights, selects, want_avg, timed, want_scores)

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
        return self._batch_round(targets, weights, selects, want_avg, timed, want_scores, set_ids)

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
    def batch_round_fit(self, queries, rows, labels, w_grids, th_grids, ballasts) -> list:
        """hyperparameter.py:57-64 for several queries of the LAST batched round (either kind) in one call and one launch
        (vq_db_batch_round_fit, include/vq_amd_round_fit.h), on the averaged similarities that round left on the device.  Per entry
        i: ``queries[i]`` the query's index in that round, ``rows[i]`` / ``labels[i]`` its labelled rows (positions in the query's
        view, as in the round's results) and their labels, ``w_grids[i]`` [G,S], ``th_grids[i]`` [T] and ``ballasts[i]``; G and T are
        common to the call.  Returns one [G,T] array per entry: the raw sums of :meth:`loss_surface` on the same similarities, bit
        for bit, for any number of labels (the caller divides by it).  An entry without labels gets None."""
        queries, rs, ys, wg, th, G, T = entry_arrays(self.S, queries, rows, labels, w_grids, th_grids, (ballasts,))
        total = int(sum(r.size for r in rs))
        with self.lock:
            Q, blk, view = self._slot_block("fit", FIT, "vq_db_batch_fit_layout", queries, G, T, total)
            pack_slots(view, Q, queries,
                       [("w_grid", np.float64, (G, 8), wg), ("th_grid", np.float64, (T,), th), ("ballast", np.float64, (), [float(b) for b in ballasts]),
                        ("L", np.int64, (), [r.size for r in rs])],
                       [("rows", np.int64, 1, rs), ("labels", np.float64, 1, ys)])
            call("vq_db_batch_round_fit", self._h, Q, G, T, total, C.c_void_p(blk.ptr), blk.nbytes)
            surface = view("surface", np.float64, (Q, G, T))
            return [surface[q] if r.size else None for q, r in zip(queries, rs)]

    def batch_round_grid(self, queries, rows, w_grids) -> list:
        """hyperparameter.py:57-58 on chosen rows for several queries of the LAST batched round (either kind) in one call and one
        launch (vq_db_batch_round_grid, include/vq_amd_round_grid.h): per entry i, the scores of ``rows[i]`` (positions in the view
        of query ``queries[i]`` of that round, as in its results; a row may repeat) under each weight of ``w_grids[i]`` [G,S], on the
        averaged similarities the round left on the device; G is common to the call.  Returns one [G, L_i] array per entry -- the bits
        of :meth:`scores_grid` on the same similarities, and with the round's (or the rescore's) weights the bits of that round's own
        scores at those rows -- and None for an entry without rows.  What a row-sharded database combines into its weight fit."""
        queries, rs, _ys, wg, _th, G, _T = entry_arrays(self.S, queries, rows, w_grids=w_grids)
        total = int(sum(r.size for r in rs))
        with self.lock:
            Q, blk, view = self._slot_block("grid", GRID, "vq_db_batch_grid_layout", queries, G, total)
            first, = pack_slots(view, Q, queries, [("w_grid", np.float64, (G, 8), wg), ("L", np.int64, (), [r.size for r in rs])],
                                [("rows", np.int64, 1, rs)])
            call("vq_db_batch_round_grid", self._h, Q, G, total, C.c_void_p(blk.ptr), blk.nbytes)
            return [view("graded", np.float64, (G, r.size), G * at) if r.size else None for r, at in zip(rs, first)]

    def batch_round_avg_rows(self, queries, rows) -> list:
        """The averaged similarities of chosen rows of several queries of the LAST batched round (either kind) in one call and one
        launch (vq_db_batch_round_avg_rows, include/vq_amd_round_shard.h): per entry i, ``avg[rows[i]]`` of query ``queries[i]`` of that
        round (positions in the query's view, as in its results; a row may repeat) as the round left them on the device -- copies,
        bit for bit, NaN payloads and the sign of zero included.  Returns one [L_i, S] array per entry, None for an entry without
        rows.  What the ranks of a row-sharded database exchange in front of :meth:`batch_round_update_given`."""
        queries, rs = entry_arrays(self.S, queries, rows)[:2]
        total = int(sum(r.size for r in rs))
        with self.lock:
            Q, blk, view = self._slot_block("grid", AVG_ROWS, "vq_db_batch_avg_rows_layout", queries, total)
            first, = pack_slots(view, Q, queries, [("L", np.int64, (), [r.size for r in rs])], [("rows", np.int64, 1, rs)])
            call("vq_db_batch_round_avg_rows", self._h, Q, total, C.c_void_p(blk.ptr), blk.nbytes)
            return [view("avg_rows", np.float64, (r.size, self.S), self.S * at) if r.size else None for r, at in zip(rs, first)]

    # ------------------------------------------------------------------ the bootstrapped targets of a group of tickets
    def batch_targets_lds_rows(self) -> int:
        """The largest draw (rows) whose systems ``batch_targets`` solves in a workgroup's local memory; longer draws solve in a
        scratch area in device memory (the library's constant, read through vq_db_batch_targets_layout)."""
        return self._layout(TARGETS, "vq_db_batch_targets_layout", 1, 1, 1, 1)["lds_rows"]

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
            off = self._layout(TARGETS, "vq_db_batch_targets_layout", Q, n_rows, n_draws, n_entries)
            blk = self.blocks.take("targets", off["bytes"])
            view = self._block_view(blk.bytes(), off)
            q_in, p_in = view("query", np.int32, (Q, 8)), view("param", np.float64, (Q, 4))
            r_in, d_in, e_in = view("rows", np.int64, (n_rows,)), view("draw", np.int32, (n_draws, 2)), view("pos", np.int32, (n_entries,))
            prev_in = view("previous", np.float64, (Q, self.S, self.E, self.D))
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
            status = view("status", np.int32, (Q, 4))
            target = view("target", np.float64, (Q, self.S, self.E, self.D))
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
            last = self._bround_last
            if last is None or max(queries) >= last.Q:
                # no batched round, or a query it did not have: the library's own refusal (VQ_E_STATE), which reads nothing of the block
                blk = self.blocks.take("fit", 64)
                call("vq_db_batch_round_rescore", self._h, sum(1 << q for q in queries), C.c_void_p(blk.ptr), blk.nbytes, flags)
                raise _lib.VqError(-4, "the last batched round does not have queries %r" % (queries,))
            blk = last.block(self.blocks)
            view = self._block_view(blk.bytes(), last.off)
            self._fill_round_inputs(view, last.Q, queries, w, bands)
            call("vq_db_batch_round_rescore", self._h, sum(1 << q for q in queries), C.c_void_p(blk.ptr), blk.nbytes, flags)
            decode = self._partition_decoder(view, last.off, last.Q)
            out = []
            for q in queries:
                r = RoundResult()
                r.avg, r.n_e = last.sims[q]
                r.scores = view("scores", np.float64, (last.rows(q),), last.start[q])
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
        given = surfaces is not None
        row_t, width = (np.float64, self.S) if tables else (np.int64, 1)
        queries = list(queries)
        eps = [float(eps)] * len(queries) if np.ndim(eps) == 0 else [float(e) for e in eps]
        if given and want_surface:
            raise ValueError("a surface that is given does not come back")
        counted = (ballasts, seconds, eps, reaches, user_rows) + ((rows, labels, surfaces) if given else ())
        queries, rs, ys, wg, th, G, T = entry_arrays(self.S, queries, None if given else rows, None if given else labels, w_grids, th_grids, counted,
                                                     row_t, width)
        k = len(queries)
        if given:
            counts = [int(y) if np.ndim(y) == 0 else len(y) for y in labels]
            rs, ys = [np.zeros(0, dtype=np.int64)] * k, [np.zeros(0)] * k
        else:
            counts = [r.size // width for r in rs]
        us = [np.zeros(0, dtype=row_t) if u is None else np.asarray(u, dtype=row_t).reshape(-1) for u in user_rows]
        if any(u.size % width for u in us):
            raise ValueError("user rows must be [., %d] averaged similarities" % self.S)
        sf = [np.asarray(f, dtype=np.float64) for f in surfaces] if given else None
        if given and any(f.shape != (G, T) for f in sf):
            raise ValueError("surfaces must be [G,T]")
        if max(queries) >= 16:
            raise ValueError("a query is its index in the last batched round")
        flags = _lib.VQ_BROUND_SELECT | (_lib.VQ_BROUND_SCORES if want_scores else 0) | (_lib.VQ_BUPDATE_SURFACE if want_surface else 0) \
            | (_lib.VQ_BUPDATE_GIVEN_SURFACE if given else 0)
        with self.lock:
            total, total_u = int(sum(y.size for y in ys)), int(sum(u.size for u in us)) // width
            Q, ublk, view = self._slot_block("update", UPDATE, "vq_db_batch_update_given_layout" if tables else "vq_db_batch_update_layout", queries,
                                             G, T, total, total_u)
            ublk.bytes()[:view.off["surface"]] = 0            # everything but the surface, whose bytes are given or the fit's
            ublk.bytes()[view.off["second"]:] = 0
            surface = view("surface", np.float64, (Q, G, T))
            pack_slots(view, Q, queries,
                       [("w_grid", np.float64, (G, 8), wg), ("th_grid", np.float64, (T,), th), ("ballast", np.float64, (), [float(b) for b in ballasts]),
                        ("L", np.int64, (), counts), ("second", np.int32, (), [int(s) for s in seconds]), ("eps", np.float64, (), eps),
                        ("band_mode", np.int32, (), [int(v is None) for v in reaches]), ("near", np.float64, (), [0.0 if v is None else float(v) for v in reaches]),
                        ("U", np.int64, (), [u.size // width for u in us])],
                       [("rows", row_t, width, rs), ("labels", np.float64, 1, ys), ("user_rows", row_t, width, us)])
            for q, f in zip(queries, sf or ()):
                surface[q] = f
            last = self._bround_last
            if last is None or max(queries) >= last.Q:
                # no batched round, or a query it did not have: VQ_E_STATE as the library gives it, also for an entry without labels
                # (a slot the library would skip) -- there is no block of that round to hand it
                raise _lib.VqError(-4, "no batched round has run on this handle" if last is None else
                                   "the last batched round had %d queries (asked for %r)" % (last.Q, queries))
            blk = last.block(self.blocks)
            rview = self._block_view(blk.bytes(), last.off)
            call("vq_db_batch_round_update_given" if tables else "vq_db_batch_round_update", self._h, Q, G, T, total, total_u, C.c_void_p(ublk.ptr),
                 ublk.nbytes, C.c_void_p(blk.ptr), blk.nbytes, flags)
            pick, idx = view("pick", np.float64, (Q, 8)), view("pick_idx", np.int32, (Q, 4))
            decode = self._partition_decoder(rview, last.off, last.Q)
            out = []
            for i, q in enumerate(queries):
                r = UpdateResult()
                served = counts[i] > 0                        # a slot without labels is skipped: it stays what the round left
                r.avg, r.n_e = last.sims[q]
                r.scores = rview("scores", np.float64, (last.rows(q),), last.start[q]) if want_scores and served else None
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
        return self._layout(TOPK, "vq_db_batch_topk_layout", 1, 1)["cap"]

    def batch_round_topk(self, ks, queries=None) -> list:
        """ticket.py:266 for several queries of the LAST batched round (either kind, whether or not it copied its scores back) in ONE
        call (vq_db_batch_round_topk, include/vq_amd_round_topk.h): the ``ks[i]`` best clips of query ``queries[i]`` of that round
        (``queries`` None: all of them, in order; ``ks`` an int: the same k for each), ranked on the device from the scores the
        round -- or a :meth:`batch_round_rescore` behind it -- left there.  One (rows, vals) per entry, as :meth:`topk` gives them:
        positions in the query's view (as in every result of that round) by descending score, ties by ascending position, NaN
        excluded, and the scores at those positions bit for bit.  A k above the rows of the query's view is clamped to them; one
        above :meth:`batch_topk_cap` is the library's refusal.  Without a batched round: ``VqError`` (VQ_E_STATE)."""
        with self.lock:
            last = self._bround_last
            if queries is None:
                queries = list(range(last.Q)) if last is not None else [0]
            queries = [int(q) for q in queries]
            n = len(queries)
            kk = [int(ks)] * n if np.ndim(ks) == 0 else [int(v) for v in ks]
            if not n or len(kk) != n or len(set(queries)) != n or min(queries) < 0 or max(queries) >= 16:
                raise ValueError("one k per query (or one int), every query -- its index in the last batched round -- once")
            if min(kk) < 0:
                raise ValueError("k must not be negative")
            if last is not None:                              # min(k, M_q); a query the round did not have keeps its k: the library refuses it
                kk = [min(k, last.rows(q)) if q < last.Q else max(k, 1) for k, q in zip(kk, queries)]
            k_max = max(max(kk), 1)
            Q, blk, view = self._slot_block("topk", TOPK, "vq_db_batch_topk_layout", queries, k_max)
            pack_slots(view, Q, queries, [("k", np.int64, (), kk), ("count", np.int64, (), ())])
            call("vq_db_batch_round_topk", self._h, Q, k_max, C.c_void_p(blk.ptr), blk.nbytes)
            count = view("count", np.int64, (Q,))
            rows, vals = view("rows", np.int64, (Q, k_max)), view("vals", np.float64, (Q, k_max))
            return [(rows[q, :int(count[q])], vals[q, :int(count[q])]) for q in queries]
