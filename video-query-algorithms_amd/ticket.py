"""Drop-in for the scoring methods of the reference's ``Ticket`` (src/models/ticket.py).

``TicketScoring`` carries the four hot-path methods with the reference's names, arguments and
result attributes -- ``compute_similarities`` (ticket.py:120-163), ``compute_scores``
(ticket.py:165-180), ``select_clips_to_review`` (ticket.py:311-356) and
``lowest_scoring_user_match`` (ticket.py:301-309) -- running on a resident :class:`FeatureDB`
through the HIP kernels.  The REST / reporting methods of the reference class are untouched: mix
this class in front of it (``class Ticket(TicketScoring, ReferenceTicket)``) or call
:func:`install` on the reference's classes.  ``Ticket`` below is a self-contained
variant for offline use whose ``_request`` answers from in-memory records.
"""
from __future__ import annotations

import contextlib
import logging
import os
import random
from collections.abc import Mapping

import numpy as np

from .feature_db import FeatureDB, whole_view


class ScoreMap(Mapping):
    """``{video_clip_id: score}`` backed by the arrays read back from the device; iteration order is
    the order in which the reference would have inserted the clips (ticket.py:146-160)."""

    def __init__(self, clip_ids: np.ndarray, values: np.ndarray, row_of):
        self._ids, self._vals, self._row_of = clip_ids, values, row_of

    def __getitem__(self, clip):
        return self._vals[self._row_of(clip)]

    def __iter__(self):
        return iter(self._ids.tolist())

    def __len__(self):
        return self._ids.shape[0]

    def __contains__(self, clip):
        try:
            self._row_of(clip)
            return True
        except (KeyError, TypeError, ValueError):
            return False

    def items(self):
        return _Pairs(self._ids, self._vals)

    def values(self):
        return list(self._vals)


class _Pairs:
    def __init__(self, ids, vals):
        self._ids, self._vals = ids, vals

    def __iter__(self):
        return zip(self._ids.tolist(), self._vals)

    def __len__(self):
        return self._ids.shape[0]


class SimilarityMap(Mapping):
    """``{video_clip_id: {stream: [avg similarity, ensemble size]}}`` (ticket.py:123-124)."""

    def __init__(self, clip_ids, streams, avg, n_e, row_of):
        self._ids, self._streams, self._avg, self._ne, self._row_of = clip_ids, streams, avg, n_e, row_of

    def _entry(self, row):
        return {st: [self._avg[row, s], int(self._ne[row, s])]
                for s, st in enumerate(self._streams) if self._ne[row, s] > 0}

    def __getitem__(self, clip):
        return self._entry(self._row_of(clip))

    def __iter__(self):
        return iter(self._ids.tolist())

    def __len__(self):
        return self._ids.shape[0]

    def items(self):
        return ((int(c), self._entry(r)) for r, c in enumerate(self._ids.tolist()))


def _user_match_rows(ticket):
    """The positions, in the ticket's search set, of the clips the user confirmed, ascending: what ``lowest_scoring_user_match``
    walks, and what a finalize member of a group hands the device for its review band (``_update_group``).  A function of this
    module, not a method: ``install`` copies only the reference's own method names onto its Ticket class."""
    view = ticket._view
    return sorted(view.row_of(int(c)) for c, v in ticket.user_matches.items()
                  if v is True and view.has_clip(c) and str(int(c)) == c)


def _db_lock(db):
    """The database's re-entrant lock (FeatureDB / ShardedFeatureDB); a database object without one gets no locking."""
    return getattr(db, "lock", None) or contextlib.nullcontext()


def _query_arrays(ticket, db):
    """(stream names, query array [S,E,D] fp64, slots in use [S,E]) of a ticket's target on database ``db``."""
    target_features = ticket.target.target_features
    stream_names = getattr(db, "stream_names", None) or list(target_features.keys())
    slot_splits = getattr(db, "slot_splits", None) or [list(target_features[st].keys()) for st in stream_names]
    # The target's vectors are Python lists (JSON-serialisable, ticket.py:296): turning 6 x 1 024 floats into an array is ~0.15 ms
    # of interpreter time, more than the whole device side of a 10k-clip round.  The array is kept on the target object and
    # reused while every vector IS the list object it was made from (TargetClip replaces a vector by a new list whenever it
    # changes it -- target_clip.py never assigns into one).
    refs = tuple(target_features[st][sp] for s, st in enumerate(stream_names) for sp in slot_splits[s]
                 if st in target_features and sp in target_features[st])
    cached = getattr(ticket.target, "_vq_query_array", None)
    if cached is not None and cached[0] == (db.S, db.E, db.D) and len(cached[1]) == len(refs) and all(a is b for a, b in zip(cached[1], refs)):
        t, slot_used = cached[2], cached[3]
    else:
        t = np.zeros((db.S, db.E, db.D), dtype=np.float64)
        slot_used = np.zeros((db.S, db.E), dtype=bool)
        for s, st in enumerate(stream_names):
            for e, sp in enumerate(slot_splits[s]):
                if st in target_features and sp in target_features[st]:
                    t[s, e] = np.asarray(target_features[st][sp], dtype=np.float64)
                    slot_used[s, e] = True
        try:
            ticket.target._vq_query_array = ((db.S, db.E, db.D), refs, t, slot_used)
        except AttributeError:
            pass                                          # a target object that takes no attributes
    return stream_names, t, slot_used


class TicketScoring:
    """Hot-path methods of the reference's Ticket, on the GPU.  Attributes read: ``target``
    (``target_features``, ``splits``), ``search_set``, ``ref_clip_id``, ``user_matches``; attributes
    written: ``similarities``, ``scores``, ``matches`` -- as in the reference."""

    feature_db: FeatureDB | None = None      # a resident DB may be attached up front
    _ahead = None                            # scores / review partition this round's compute_similarities or compute_scores already brought back
    _hp = None                               # the hyperparameters object of the latest compute_similarities
    _stream_gap = None                       # per stream: does any clip lack it (compute_scores' KeyError of ticket.py:177)
    _round = None                            # token of this ticket's latest compute_similarities (see _own_similarities)
    _score_weights = None
    _view = None                             # the search-set view this round is bound to (feature_db.SearchSetView)
    _fit = None                              # (weights, threshold) fitted behind a batched pass (compute_similarities_batch(fit=))
    _fit_round = None                        # the _round token that fit belongs to
    _top = None                              # (clip ids, scores) of the best clips, ranked behind a pass (compute_similarities_batch(top=))
    _top_round = None                        # the _round token that ranking belongs to
    _top_weights = None                      # the score weights (bytes) it was taken under
    feature_db_dtype = np.float64            # dtype used when the DB is built from API records
    device = 0

    # -- ticket.py:120-163 ------------------------------------------------------------------
    def compute_similarities(self, hyperparameters):
        target_features = self.target.target_features
        db = self.feature_db
        if db is None:
            records = self._request(["search-sets", "features"], {"id": self.search_set})   # ticket.py:363-365
            db = FeatureDB.from_records(records, target_features, hyperparameters.streams,
                                        hyperparameters.feature_name, dtype=self.feature_db_dtype,
                                        device=self.device)
            self.feature_db = db
        stream_names, t, slot_used = _query_arrays(self, db)
        self._ahead = None
        with _db_lock(db):                    # one resident database may serve several tickets: these calls are one step
            # The clips of THIS ticket's search set (ticket.py:363-365), when the resident database has it defined: the round runs
            # over that view and everything below is indexed by position in it.  The ticket keeps the view OBJECT -- the set the
            # handle has in use is shared state that the next ticket changes.
            view = self._bind_view(db)
            db.restrict_slots(slot_used)      # per query; the database's own mask is never modified (no device call unless it changes)
            self._round = object()            # whose similarities the database holds now (see _own_similarities)
            ahead = self._look_ahead(hyperparameters, stream_names) if hasattr(db, "query_round") else None
            if ahead is not None:
                # The round in ONE call (vq_db_query_round): the reference calls compute_scores and select_clips_to_review right behind
                # this method (compute_matches.py:58-89) with the weights / threshold its hyperparameters object holds now, so scores and
                # review partition are computed and brought back with the similarities; compute_scores / select_clips_to_review use
                # them when they are called with exactly those arguments and run their own calls otherwise.
                w, th, lower = ahead
                r = db.query_round(t, weights=w, select=(th, lower))
                avg, n_e = r.avg, r.n_e
                self._ahead = {"w": w.tobytes(), "scores": r.scores, "select": (th, lower), "match_rows": r.match_rows,
                               "near_rows": r.near_rows, "near_argmax": r.near_argmax}
                db.sims_owner, db.scores_owner = self._round, (self._round, w.tobytes())
            else:
                db.set_query(t)
                db.scan(weights=None)
                avg, n_e = db.similarities()
                db.sims_owner, db.scores_owner = self._round, None
        self._hp = hyperparameters
        self._stream_names = stream_names
        self._avg, self._n_e = avg, n_e
        self._stream_gap = None
        self._view = view
        self.similarities = SimilarityMap(view.clip_ids, stream_names, avg, n_e, view.row_of)

    def _bind_view(self, db):
        """Select this ticket's search set on the database (no call when it is the one in use) and return its view; a database
        without that set defined -- or without search sets at all -- is scanned whole, as ever.  Call with the lock held."""
        if not hasattr(db, "use_search_set"):
            return whole_view(db)
        set_id = getattr(self, "search_set", None)
        return db.use_search_set(set_id if db.has_search_set(set_id) else None)

    @staticmethod
    def _review_band(hyperparameters):
        """(threshold, lower limit) select_clips_to_review will most likely be called with (compute_matches.py:78-88)."""
        th = getattr(hyperparameters, "threshold", None)
        if th is None:
            th = getattr(hyperparameters, "default_threshold", None)
        near = getattr(hyperparameters, "near_miss_default", None)
        if th is None or near is None:
            return None
        return float(th), float(th) - float(near) * (1 - float(th))          # the expression of ticket.py:316

    def _look_ahead(self, hyperparameters, stream_names):
        """The arguments compute_scores / select_clips_to_review are about to get if the caller is the reference's compute_matches:
        (weights [S], threshold, lower limit), or None when the hyperparameters object does not say."""
        weights = getattr(hyperparameters, "weights", None) or getattr(hyperparameters, "default_weights", None)
        band = self._review_band(hyperparameters)
        if not isinstance(weights, Mapping) or band is None:
            return None
        w = np.zeros(len(stream_names), dtype=np.float64)
        for stream_type, ws in weights.items():
            if stream_type not in stream_names:
                return None
            w[stream_names.index(stream_type)] = ws
        return w, band[0], band[1]

    # -- ticket.py:165-180 ------------------------------------------------------------------
    def compute_scores(self, weights):
        db = self.feature_db
        w = np.zeros(db.S, dtype=np.float64)
        if self._stream_gap is None:                 # stream -> does some clip have no similarity for it: one pass per round and stream
            self._stream_gap = {}
        for stream_type, ws in weights.items():
            s = self._stream_names.index(stream_type) if stream_type in self._stream_names else -1
            if s >= 0 and s not in self._stream_gap:
                self._stream_gap[s] = bool((self._n_e[:, s] == 0).any())
            if s < 0 or self._stream_gap[s]:
                raise KeyError(stream_type)          # vsim[stream_type] at ticket.py:177
            w[s] = ws
        ahead = getattr(self, "_ahead", None)
        if ahead is not None and ahead["w"] == w.tobytes():
            # computed from THIS round's similarities under exactly these weights and already on the host: nothing to ask the device
            # (whose scores may meanwhile be another ticket's: select_clips_to_review / _own_scores look after that)
            self._score_values = ahead["scores"]
            self._score_weights = w
            self.scores = ScoreMap(self._view.clip_ids, self._score_values, self._view.row_of)
            return
        with _db_lock(db):
            self._own_similarities()
            band = self._review_band(getattr(self, "_hp", None)) if hasattr(db, "query_round") else None
            if band is not None:                               # re-weighting + the partition select_clips_to_review is about to ask for
                r = db.query_round(None, weights=w, select=band)
                self._score_values = r.scores
                self._ahead = {"w": w.tobytes(), "scores": r.scores, "select": band, "match_rows": r.match_rows,
                               "near_rows": r.near_rows, "near_argmax": r.near_argmax}
            else:
                db.rescore(w)
                self._score_values = db.scores()
                self._ahead = None
            self._score_weights = w
            db.scores_owner = (self._round, w.tobytes())
        self.scores = ScoreMap(self._view.clip_ids, self._score_values, self._view.row_of)

    # -- a resident database shared between tickets -------------------------------------------------
    def _own_similarities(self):
        """The query, the averaged similarities and the scores are state of the database HANDLE, and a round is several calls
        (compute_similarities, optimize_weights, compute_scores, select_clips_to_review -- compute_matches.py:58-89).  When another
        ticket used the same resident database in between, this ticket's averaged similarities (kept on the host since
        compute_similarities) go back to the device before anything is computed from them: N x S x 12 bytes, only ever on a
        collision -- after this ticket's search set has been selected again (the other ticket's round ran over its own).  Call with
        the database's lock held."""
        db = self.feature_db
        if getattr(db, "sims_owner", self._round) is not self._round:
            if hasattr(db, "use_search_set"):
                db.use_search_set(self._view.set_id)
            db.write_avg(self._avg, self._n_e)
            db.sims_owner, db.scores_owner = self._round, None

    def _own_scores(self):
        """As above for the scores the selection kernels read: recomputed from this ticket's similarities and its last weights
        when the device holds somebody else's."""
        db = self.feature_db
        mine = (self._round, self._score_weights.tobytes())
        if getattr(db, "scores_owner", mine) != mine:
            self._own_similarities()
            db.rescore(self._score_weights)
            db.scores_owner = mine

    # -- ticket.py:266 (the report's order) on the whole search set --------------------------------
    def top_clips(self, k):
        """(clip ids, scores) of the ``k`` best clips of this round under the ticket's current score weights: descending score, ties
        in search-set order, clips without a score left out.  Served from the ranking ``compute_similarities_batch(top=)`` took with
        the pass when that belongs to this round, holds enough entries and was taken under these weights; otherwise the database
        ranks the ticket's scores (``topk``) under its lock."""
        k = int(k)
        top, w = self._top, self._score_weights
        if top is not None and self._round is not None and self._top_round is self._round and len(top[0]) >= min(k, self._view.n) \
                and (w is None or w.tobytes() == self._top_weights):   # no compute_scores yet: the scores are the look-ahead ones
            return top[0][:k], top[1][:k]
        db = self.feature_db
        with _db_lock(db):
            self._own_scores()
            rows, vals = db.topk(k)
            return self._view.clip_ids[rows], np.array(vals)

    # -- ticket.py:301-309 ------------------------------------------------------------------
    def lowest_scoring_user_match(self):
        view = self._view                            # positions in the ticket's search set
        rows = _user_match_rows(self)
        min_score, min_clip = 1, None
        for r in rows:                               # same order as the walk over self.scores
            min_score = min(min_score, self._score_values[r])
            min_clip = int(view.clip_ids[r])
        return min_score, min_clip

    # -- ticket.py:311-356 ------------------------------------------------------------------
    def select_clips_to_review(self, threshold=0.8, max_number_matches=20, near_miss=0.5):
        db = self.feature_db
        vals, ids = self._score_values, self._view.clip_ids
        lower_limit = threshold - near_miss * (1 - threshold)
        ahead = getattr(self, "_ahead", None)
        if ahead is not None and ahead["select"] == (threshold, lower_limit) and ahead["w"] == self._score_weights.tobytes():
            # the partition of exactly these scores under exactly this band came back with them
            match_rows, near_rows, near_argmax = ahead["match_rows"], ahead["near_rows"], ahead["near_argmax"]
        else:
            with _db_lock(db):
                self._own_scores()
                match_rows, near_rows, near_argmax = db.select(threshold, lower_limit)     # stable partition on the GPU
        mscores = int(min(max_number_matches / 2, len(match_rows)))
        m_near_scores = int(min(max_number_matches - mscores, len(near_rows)))
        # random.sample draws positions from (len(population), k) only, so sampling positions
        # consumes the generator exactly like sampling the (clip, score) pairs (ticket.py:333,341)
        picked = [match_rows[j] for j in random.sample(range(len(match_rows)), mscores)]
        near_max_row = None
        if m_near_scores > 0:
            m_near_scores -= 1
            near_max_row = near_argmax                                                 # first max in order
            near_rows = near_rows[near_rows != near_argmax]
        picked += [near_rows[j] for j in random.sample(range(len(near_rows)), m_near_scores)]
        matches = {int(ids[r]): vals[r] for r in picked}
        if near_max_row is not None:
            matches[int(ids[near_max_row])] = vals[near_max_row]
        # clips the user has already judged stay in the review set whatever their score: the reference clip (when it is
        # part of the search set) and every confirmed match (ticket.py:346-356); a confirmed match that is not in the
        # search set is a KeyError there and here
        forced = [self.ref_clip_id] if self.ref_clip_id in self.scores else []
        forced += [int(clip) for clip, verdict in (self.user_matches or {}).items() if verdict is True]
        for clip in forced:
            matches[clip] = self.scores[clip]
        self.matches = matches


# -- several tickets in one pass over a resident database -----------------------------------------------------------------------------
BATCH_PASS = 16       # queries per pass of the batched round (include/vq_amd_rounds.h)
# share_search_sets: a group with search-set members shares ONE pass over the union of their sets (include/vq_amd_round_views.h) when
# sum M_q >= SHARE_SETS_FACTOR * distinct, M_q = the members' set sizes (N for a whole-database member) and distinct = min(N, sum of M
# over the distinct set ids of the group).  `distinct` bounds the rows the union can hold, so a shared pass then reads at most half
# the rows the members' own rounds would read.  The two kernels run at 0.75 (16-query pass) against 0.85 (one-query scan) of the HBM
# peak (README), which puts break-even near sum M_q = 1.13 |U|: well inside the factor of 2, and the rule needs no union on the host.
SHARE_SETS_FACTOR = 2


def _batchable(ticket, hyperparameters, share_search_sets=False):
    """(database, stream names, query, slots in use, look-ahead) when the ticket's round can share a 16-query pass, else None: it has
    a resident database with ``query_round_batch`` that meets the pass's preconditions, runs over the WHOLE database (no search set
    defined for it) and its hyperparameters say which weights and band come next."""
    db = ticket.feature_db
    if db is None or not hasattr(db, "query_round_batch"):
        return None
    if hasattr(db, "has_search_set") and db.has_search_set(getattr(ticket, "search_set", None)):
        if not (share_search_sets and hasattr(db, "query_round_batch_sets")):
            return None
    supported = getattr(db, "batch_round_supported", None)
    if supported is not None and not supported():
        return None
    stream_names, t, slot_used = _query_arrays(ticket, db)
    ahead = ticket._look_ahead(hyperparameters, stream_names)
    if ahead is None:
        return None
    return db, stream_names, t, slot_used, ahead


def _adopt(group, views, results):
    """Every member of a pass gets the attributes its own compute_similarities sets, from its result of the pass."""
    for (tk, hp, prep, _fit), view, r in zip(group, views, results):
        _db, stream_names, _t, _used, (w, th, lower) = prep
        tk._round = object()
        tk._ahead = {"w": w.tobytes(), "scores": r.scores, "select": (th, lower), "match_rows": r.match_rows,
                     "near_rows": r.near_rows, "near_argmax": r.near_argmax}
        tk._hp = hp
        tk._stream_names = stream_names
        tk._avg, tk._n_e = r.avg, r.n_e
        tk._stream_gap = None
        tk._view = view
        tk.similarities = SimilarityMap(view.clip_ids, stream_names, r.avg, r.n_e, view.row_of)


def _fit_group(db, group):
    """The weight update of the members with ``fit`` set (hyperparameter.py:29-76, then compute_matches.py:77-88) on the averaged
    similarities their pass left on the device: ONE ``batch_round_fit`` for the loss surfaces of all of them, the pick on the host
    (``Hyperparameter._pick_from``), ONE ``batch_round_rescore`` under the fitted weights and the review band of the fitted
    threshold.  Such a ticket ends with ``_fit`` = (weights, threshold) for this round and ``_ahead`` = the rescore's scores and
    partition.  A member without labelled clips, with a label on an unknown clip (optimize_weights raises that in its own place) or
    with grids of another size than the first one's stays as the pass left it; so does every member on a database without the two
    methods.  Members marked ``_OnDevice`` (``fit_on_device``) on a database with ``batch_round_update`` -- a ``FeatureDB``, or a
    ``ShardedFeatureDB`` with batched rounds -- take ``_update_group`` instead: one call for all of it.  Call behind the group's own pass with the database's lock still held: the next pass on the
    handle replaces what this reads."""
    on_device = hasattr(db, "batch_round_update") and any(isinstance(fit, _OnDevice) for _tk, _hp, _prep, fit in group)
    if not on_device and not (hasattr(db, "batch_round_fit") and hasattr(db, "batch_round_rescore")):
        return
    members = []
    for q, (tk, hp, prep, fit) in enumerate(group):
        if not fit or not hasattr(hp, "_pick_from"):
            continue
        try:
            rows, labels = hp._labelled_rows(tk)
            first, second = (prep[1].index(st) for st in hp.streams[:2])
        except (KeyError, ValueError):
            continue
        if not rows or (members and (len(hp.weight_grid), len(hp.threshold_grid)) != members[0][5].shape[:1] + members[0][6].shape):
            continue
        candidates = np.zeros((len(hp.weight_grid), db.S))
        candidates[:, first], candidates[:, second] = 1.0, hp.weight_grid
        members.append((q, tk, hp, rows, [float(v) for v in labels], candidates, np.asarray(hp.threshold_grid, dtype=np.float64), second,
                        getattr(fit, "finalize", False)))
    if not members:
        return
    if on_device:
        _update_group(db, members)
        return
    surfaces = db.batch_round_fit([m[0] for m in members], [m[3] for m in members], [m[4] for m in members], [m[5] for m in members],
                                  [m[6] for m in members], [m[2].ballast for m in members])
    fits, weights, bands = [], [], []
    for (q, tk, hp, rows, labels, _cand, _ths, _second, _finalize), surface in zip(members, surfaces):
        picked, th = hp._pick_from(np.asarray(surface) / len(labels))
        w = np.zeros(db.S, dtype=np.float64)                          # as compute_scores builds it from the dict
        for stream_type, ws in picked.items():
            w[tk._stream_names.index(stream_type)] = ws
        fits.append((picked, th))
        weights.append(w)
        bands.append((float(th), float(th) - float(hp.near_miss_default) * (1 - float(th))))       # _review_band's expression
    results = db.batch_round_rescore([m[0] for m in members], np.stack(weights), np.array(bands, dtype=np.float64))
    for (q, tk, _hp, _rows, _labels, _cand, _ths, _second, _finalize), fit, w, band, r in zip(members, fits, weights, bands, results):
        tk._ahead = {"w": w.tobytes(), "scores": r.scores, "select": band, "match_rows": r.match_rows, "near_rows": r.near_rows,
                     "near_argmax": r.near_argmax}
        tk._fit, tk._fit_round = fit, tk._round


class _OnDevice:
    """The ``fit`` entry of a group member under ``fit_on_device``: true like the plain flag, and it says which band the member wants
    (``_fit_group`` reads it into the member's own tuple)."""
    __slots__ = ("finalize",)

    def __init__(self, finalize):
        self.finalize = bool(finalize)


def _update_group(db, members):
    """``_fit_group`` in ONE ``batch_round_update``: surfaces, the pick (``Hyperparameter._pick_exact``'s, not ``_pick_from``'s: the one
    difference of the mode), the rescore, the band and the partition without a host step in between.  A revise member's band reaches
    ``near_miss_default`` below its threshold; a finalize member's reaches the lowest score among the user's confirmed matches
    (``lowest_scoring_user_match``'s rows, ``compute_matches._review_budget``'s expressions), so its ``select_clips_to_review`` finds the
    partition in ``_ahead`` as a revise member's does.  On a ``ShardedFeatureDB`` the rows and user rows are positions in the whole
    database's view, which are its global row numbers: what ``ShardedFeatureDB.batch_round_update`` takes."""
    reaches = [None if m[8] else float(m[2].near_miss_default) for m in members]
    # a finalize member without user matches reaches nowhere (lowest 1.0); lowest_scoring_user_match raises later where it always did
    user_rows = [_user_match_rows(m[1]) if m[8] and m[1].user_matches else [] for m in members]
    results = db.batch_round_update([m[0] for m in members], [m[3] for m in members], [m[4] for m in members], [m[5] for m in members],
                                    [m[6] for m in members], [m[2].ballast for m in members], [m[7] for m in members],
                                    float(os.environ["COMPUTE_EPS"]), reaches, user_rows)
    for (q, tk, hp, _rows, _labels, _cand, _ths, _second, _finalize), r in zip(members, results):
        if r.fell_back:                                               # the warning of Hyperparameter._refine
            logging.warning("hyperparameter quadratic fine tuning failed - resort to selecting optimum on grid "
                            "without further interpolation")
        picked = {hp.streams[0]: 1.0, hp.streams[1]: r.w}
        w = np.zeros(db.S, dtype=np.float64)                          # as compute_scores builds it from the dict
        for stream_type, ws in picked.items():
            w[tk._stream_names.index(stream_type)] = ws
        tk._ahead = {"w": w.tobytes(), "scores": r.scores, "select": r.band, "match_rows": r.match_rows, "near_rows": r.near_rows,
                     "near_argmax": r.near_argmax}
        tk._fit, tk._fit_round = (picked, r.threshold), tk._round


def _set_top(tk, rows, vals):
    """``_top`` of a ticket from positions in its view and their scores, under the weights of its look-ahead scores."""
    tk._top = (tk._view.clip_ids[np.asarray(rows, dtype=np.int64)], np.array(vals))
    tk._top_round, tk._top_weights = tk._round, tk._ahead["w"]


def _rank_group(db, group, tops):
    """The ``top`` best clips of every member of a pass (ticket.py:266 on the whole search set) in ONE ``batch_round_topk`` on the
    scores the pass -- and the rescore of ``_fit_group`` behind it -- left on the device.  Every member ends with ``_top`` = (clip
    ids, scores), ``_top_round`` = its ``_round`` and ``_top_weights`` = the weights those scores stand under (its ``_ahead``'s).
    Call behind ``_fit_group`` with the database's lock still held."""
    if tops is None or not hasattr(db, "batch_round_topk"):
        return
    ranked = db.batch_round_topk([int(k) for k in tops])
    for (tk, _hp, _prep, _fit), (rows, vals) in zip(group, ranked):
        _set_top(tk, rows, vals)


def _rank_alone(tk, k):
    """The same for a ticket that ran its own round: ``topk`` of its database, under its lock, on the look-ahead scores."""
    db = tk.feature_db
    ahead = getattr(tk, "_ahead", None)
    if k is None or db is None or ahead is None or not hasattr(db, "topk"):
        return
    with _db_lock(db):
        mine = (tk._round, ahead["w"])
        if getattr(db, "scores_owner", mine) != mine:                  # somebody else's scores on the handle by now: top_clips will ask
            return
        rows, vals = db.topk(int(k))
        _set_top(tk, rows, vals)


def _batched_pass(group, tops=None):
    """One pass for up to BATCH_PASS tickets that share a database object and a slot mask: what compute_similarities does for each,
    the look-ahead scores and partition included."""
    db, slot_used = group[0][2][0], group[0][2][3]
    targets = np.stack([g[2][2] for g in group])
    weights = np.stack([g[2][4][0] for g in group])
    bands = np.array([[g[2][4][1], g[2][4][2]] for g in group], dtype=np.float64)
    for tk, _hp, _prep, _fit in group:
        tk._ahead = None
    with _db_lock(db):
        views = [tk._bind_view(db) for tk, _hp, _prep, _fit in group]       # the whole database: no set is defined for any of them
        db.restrict_slots(slot_used)                                  # once per group
        results = db.query_round_batch(targets, weights, bands, want_avg=True)
        # the handle's one-query state is nobody's round now: a later device-side step of any of these tickets puts its
        # similarities back first (_own_similarities / _own_scores)
        db.sims_owner = db.scores_owner = None
        _adopt(group, views, results)
        _fit_group(db, group)                                         # fit=: behind its own pass, in the same hold of the lock
        _rank_group(db, group, tops)                                  # top=: behind the fit, so a fitted member ranks under its fitted weights


def _set_of(db, ticket):
    """The id of the ticket's search set if the database has it defined, else None (the whole database)."""
    set_id = getattr(ticket, "search_set", None)
    return set_id if hasattr(db, "has_search_set") and db.has_search_set(set_id) else None


def _shared_sets_pass(group, tops=None):
    """ONE pass over the union of the members' search sets (FeatureDB.query_round_batch_sets): what compute_similarities does for each
    member under its own set -- ``_view`` is its set's view, everything else is indexed by position in it."""
    db, slot_used = group[0][2][0], group[0][2][3]
    targets = np.stack([g[2][2] for g in group])
    weights = np.stack([g[2][4][0] for g in group])
    bands = np.array([[g[2][4][1], g[2][4][2]] for g in group], dtype=np.float64)
    for tk, _hp, _prep, _fit in group:
        tk._ahead = None
    with _db_lock(db):
        set_ids = [_set_of(db, tk) for tk, _hp, _prep, _fit in group]
        views = [db.search_set_view(sid) for sid in set_ids]          # the view objects: the set the handle has in use stays
        db.restrict_slots(slot_used)                                  # once per group
        results = db.query_round_batch_sets(targets, weights, set_ids, bands, want_avg=True)
        db.sims_owner = db.scores_owner = None                        # as after _batched_pass: nobody's round
        _adopt(group, views, results)
        _fit_group(db, group)                                         # fit=: behind its own pass, in the same hold of the lock
        _rank_group(db, group, tops)                                  # top=: behind the fit, as in _batched_pass


def _flush(group, top_of=None):
    """Run a group of tickets that share a database object and a slot mask.  Without search-set members: one pass, or the ticket's own
    round when it is alone.  With them (share_search_sets): one pass over the union if the sharing rule holds, else the search-set
    members' own rounds in list order and the whole-database members as a group of today's kind.  ``top_of``: id(ticket) -> how many
    best clips to rank behind its round (None: no ranking)."""
    db = group[0][2][0]

    def tops(members):
        return None if top_of is None else [top_of[id(tk)] for tk, _hp, _prep, _fit in members]

    def alone(tk, hp):
        tk.compute_similarities(hp)
        if top_of is not None:
            _rank_alone(tk, top_of[id(tk)])
    set_ids = [_set_of(db, tk) for tk, _hp, _prep, _fit in group]
    if any(sid is not None for sid in set_ids):
        n = len(db.clip_ids)
        sizes = {sid: db.search_set_view(sid).n for sid in set(set_ids) if sid is not None}
        total = sum(n if sid is None else sizes[sid] for sid in set_ids)
        distinct = min(n, sum(sizes.values()) + (n if None in set_ids else 0))
        if len(group) > 1 and total >= SHARE_SETS_FACTOR * distinct:
            _shared_sets_pass(group, tops(group))
            return
        for (tk, hp, _prep, _fit), sid in zip(group, set_ids):
            if sid is not None:
                alone(tk, hp)
        group = [g for g, sid in zip(group, set_ids) if sid is None]
        if not group:
            return
    if len(group) == 1:                                   # nobody to share a pass with: the ticket's own round, bit for bit
        alone(group[0][0], group[0][1])
    else:
        _batched_pass(group, tops(group))


def compute_similarities_batch(tickets, hyperparameters, share_search_sets=False, fit=None, top=None, fit_on_device=False, finalize=None):
    """``compute_similarities`` for a list of tickets, those that can sharing passes over their resident database: a broker with
    several pending tickets pays one read of the database per 16 of them instead of one each.  ``hyperparameters`` is one object or
    one per ticket.  Every ticket ends with exactly the attributes its own ``compute_similarities`` sets (``similarities``, ``_avg``,
    ``_n_e``, ``_view``, ``_round``, ``_hp``, ``_stream_names``, ``_stream_gap``, ``_ahead`` -- look-ahead scores and partition included,
    so the ``compute_scores`` / ``select_clips_to_review`` that follow ask the device for nothing when called with the looked-ahead
    arguments); values agree with the one-ticket round to rounding (<= 1e-12: the pass runs on the matrix cores).

    Tickets share a pass when they have the same database OBJECT with ``query_round_batch`` that meets the pass's preconditions, no
    search set defined for them, the same slot mask and a look-ahead; at most 16 per pass, in list order.  Every other ticket -- on
    a ShardedFeatureDB opened without ``batch_rounds=True`` (with it the four calls of a batched round exist there too, for rounds
    over the whole database) or another database without the method, with a search set, without a resident database
    (``from_records``) -- runs its own ``compute_similarities``, in list order; so does, at the end, a ticket left alone in its group (a pass of one
    gains nothing).

    ``share_search_sets=True``: a ticket whose search set is defined on its database (which must have ``query_round_batch_sets``)
    joins its group too, keyed as ever.  A group with such members runs ONE pass over the union of the members' sets when
    sum M_q >= SHARE_SETS_FACTOR * distinct (see the constant); otherwise its search-set members run their own rounds in list order
    and its whole-database members share a pass as above.  After a shared pass every member has the attributes its own
    ``compute_similarities`` sets, ``_view`` = its set's view and rows as positions in it.

    ``fit``: one boolean per ticket.  The members of a pass with ``fit[i]`` true and at least one labelled clip (``ticket.matches``,
    read by ``Hyperparameter._labelled_rows``) get their weight update right behind the pass, on the similarities it left on the
    device (``_fit_group``): one ``batch_round_fit`` and one ``batch_round_rescore`` for the whole group instead of every ticket's
    ``write_avg``, ``loss_surface`` and two ``query_round`` calls.  Such a ticket ends with ``_fit`` = (weights dict, threshold) for
    this round -- what ``optimize_weights`` would set on its hyperparameters object, on the pass's own similarities -- and with
    ``_ahead`` rebuilt under those weights and the review band of that threshold, so ``compute_scores(weights)`` and
    ``select_clips_to_review(threshold, ., near_miss_default)`` ask the device for nothing.  Every other ticket is unchanged and its
    caller runs ``optimize_weights``: one that ran its own round, one on a database without the two methods, one without labels.

    ``fit_on_device=True`` (with ``fit`` and ``finalize``, one boolean per ticket: is it a finalize round): on a database with
    ``batch_round_update`` the group's update is ONE call -- the minimum of every surface is picked and refined on the device and a
    finalize member's review band, which reaches down to ``lowest_scoring_user_match`` under the fitted scores, is computed and
    partitioned there too, so its ``select_clips_to_review`` asks the device for nothing either.  One difference: weights and
    threshold are ``Hyperparameter._pick_exact``'s, not ``_pick_from``'s (squares as products instead of libm's ``pow``: a few ulp
    in some refined picks, tests/test_pick_exact.py).  On a ``ShardedFeatureDB`` opened with ``batch_rounds=True`` the switch means the
    same: its ``batch_round_update`` is one operation of the sharded database (the rows a ticket names on the whole database are
    GLOBAL row numbers) with the bits of the call on one GPU.  A database without the method does what it does without the switch.

    ``top``: an int, or one per ticket.  Every member of a pass also gets the ``top`` best clips of its search set, ranked on the
    device in the same hold of the lock, BEHIND the fit -- a fitted member is ranked under its fitted weights: one
    ``batch_round_topk`` per pass, so no N-sized array comes back for the ranking.  Such a ticket ends with ``_top`` = (clip ids
    [count], scores [count]) by descending score, ties in search-set order, and ``_top_round`` = its ``_round``;
    ``top_clips(k)`` serves ``k <= top`` from it while the ticket's score weights are the ones it was taken under.  A ticket that
    ran its own round gets the same from its database's ``topk`` (when it has one and the round looked ahead).  ``None``: no
    ranking; ``_top`` is left as it was and belongs to no round of this call."""
    tickets = list(tickets)
    fits = [False] * len(tickets) if fit is None else [bool(f) for f in fit]
    if len(fits) != len(tickets):
        raise ValueError("fit: one boolean per ticket")
    if fit_on_device:
        if finalize is None or len(finalize) != len(tickets):
            raise ValueError("fit_on_device: finalize must say for every ticket whether its round is a finalize round")
        fits = [_OnDevice(fin) if f else False for f, fin in zip(fits, finalize)]
    hps = list(hyperparameters) if isinstance(hyperparameters, (list, tuple)) else [hyperparameters] * len(tickets)
    if len(hps) != len(tickets):
        raise ValueError("one hyperparameters object, or one per ticket")
    top_of = None
    if top is not None:
        counts = [int(top)] * len(tickets) if np.ndim(top) == 0 else [int(k) for k in top]
        if len(counts) != len(tickets) or any(k < 1 for k in counts):
            raise ValueError("top: one positive int, or one per ticket")
        top_of = {id(tk): k for tk, k in zip(tickets, counts)}
    pending = {}                                          # (database object, slot mask) -> the tickets waiting for a pass, in list order
    for tk, hp, want_fit in zip(tickets, hps, fits):
        prep = _batchable(tk, hp, share_search_sets)
        if prep is None:
            tk.compute_similarities(hp)
            if top_of is not None:
                _rank_alone(tk, top_of[id(tk)])
            continue
        key = (id(prep[0]), prep[3].tobytes())
        group = pending.setdefault(key, [])
        group.append((tk, hp, prep, want_fit))
        if len(group) == BATCH_PASS:
            _flush(pending.pop(key), top_of)
    for group in pending.values():
        _flush(group, top_of)


class Ticket(TicketScoring):
    """Self-contained ticket for offline use: the attributes of ticket.py:38-57 plus an in-memory
    ``_request`` for the two feature endpoints the hot path calls."""

    def __init__(self, update_object, records=None, feature_db: FeatureDB | None = None, device: int = 0):
        self.query_id = update_object.get("query_id")
        self.video_id = update_object.get("video_id")
        self.ref_clip = update_object.get("ref_clip")
        self.ref_clip_id = update_object.get("ref_clip_id")
        self.search_set = update_object.get("search_set")
        self.number_of_matches_to_review = update_object.get("number_of_matches_to_review", 20)
        self.dynamic_target_adjustment = update_object.get("dynamic_target_adjustment", False)
        self.latest_query_result = update_object.get("latest_query_result")
        self.matches = update_object.get("matches", [])
        self.user_matches = update_object.get("user_matches", {})
        self.target = None
        self.similarities = {}
        self.scores = {}
        self.client = None
        self.schema = None
        self.feature_db = feature_db
        self.device = device
        self._records = records if records is not None else []
        # matches of the latest query result ({"video_clip": id, "user_match": True/False/None}), served in pages like
        # the API endpoint ["matches", "list"] that target bootstrapping reads (target_clip.py:114-121)
        self._match_list = update_object.get("match_list", [])
        self._match_page = int(update_object.get("match_page_size", 100))

    def _request(self, action, params):
        if action == ["search-sets", "features"]:
            return self._records
        if action == ["video-clips", "features"]:
            return [r for r in self._records if r["video_clip_id"] == params["id"]]
        if action == ["matches", "list"]:
            page = int(params.get("page", 1))
            chunk = self._match_list[(page - 1) * self._match_page:page * self._match_page]
            nxt = page + 1 if page * self._match_page < len(self._match_list) else None
            return {"results": chunk, "pagination": {"nextPage": nxt}}
        raise KeyError("offline Ticket has no endpoint %r" % (action,))

    # -- the REST side of a query round, kept in memory (the reference posts these to the API: ticket.py:59-118,
    #    :276-299).  Enough for ``compute_matches(query_updates, hyperparameters)`` to run with no server; what the
    #    server would have received can be read back from ``ledger``.
    @property
    def ledger(self):
        return self.__dict__.setdefault("_ledger", {"process_state": [], "notes": [], "query_results": [], "matches": [],
                                                    "final_report": None})

    def change_process_state(self, process_state, message=None):
        self.ledger["process_state"].append(process_state)
        if message:
            self.add_note(message)
        return process_state

    def add_note(self, note):
        self.ledger["notes"].append(note)

    def catch_errors(self, job_type):
        """(fatal message, warning) -- the three consistency checks of ticket.py:80-110; the third one switches
        dynamic target adjustment off for the round when the user confirmed nothing."""
        fatal, warnings = [], []
        if self.ref_clip_id is None:
            fatal.append("*** Fatal Error: A video clip corresponding to the reference time does not exist in the database. ***")
        if job_type != "new" and not self.matches:
            fatal.append("*** Fatal Error: This is not a new query but there are 0 matches computed for the previous round.")
        if job_type != "new" and self.dynamic_target_adjustment is True \
                and not any(m["user_match"] is True for m in self.matches):
            warnings.append("*** Error: Dynamic target adjustment is True but there are no user matches provided for the "
                            "previous round. Changing dynamic target adjustment to False")
            self.dynamic_target_adjustment = False
        return "\n".join(fatal), "\n".join(warnings)

    def create_query_result(self, nround, hyperparameters):
        import json
        results = self.ledger["query_results"]
        results.append({"id": len(results) + 1, "round": nround, "match_criterion": hyperparameters.threshold,
                        "weights": [hyperparameters.weights[st] for st in hyperparameters.streams], "query": self.query_id,
                        "bootstrapped_target": json.dumps(self.target.target_features)})
        return results[-1]["id"]

    def add_matches_to_database(self, new_result_id):
        for clip, score in self.matches.items():
            self.ledger["matches"].append({"query_result": new_result_id, "score": score, "video_clip": clip,
                                           "user_match": self.user_matches.get(str(clip))})

    def create_final_report(self, hyperparameters, query_result_id):
        """The rows of the report of ticket.py:244-268: every selected clip, best score first (stable)."""
        criterion = self.ledger["query_results"][query_result_id - 1]["match_criterion"]

        def kind(clip, score):
            verdict = self.user_matches.get(str(clip))
            if verdict is not None:
                return "user-identified match" if verdict is True else "user-identified non-match"
            return "inferred match" if score >= criterion else "inferred non-match"
        rows = [[clip, kind(clip, score), score] for clip, score in self.matches.items()]
        rows.sort(key=lambda row: row[2], reverse=True)
        self.ledger["final_report"] = rows


def install(ticket_cls, hyperparameter_cls=None, target_clip_cls=None):
    """Patch the reference's classes in place so broker.py / compute_matches.py see a drop-in."""
    if target_clip_cls is not None:                       # dynamic target adjustment: matrix formulas on the GPU
        from . import target_clip as _tc
        for name in _tc.GRAFTED:
            setattr(target_clip_cls, name, _tc.TargetClip.__dict__[name])      # __dict__: staticmethods stay static
        construct = target_clip_cls.__init__

        def remember_ticket(self, ticket, hyperparameters):
            construct(self, ticket, hyperparameters)
            self._ticket = ticket                          # lets the round use rows of a resident ticket.feature_db
        target_clip_cls.__init__ = remember_ticket
    for name in ("compute_similarities", "compute_scores", "lowest_scoring_user_match", "select_clips_to_review",
                 "_own_similarities", "_own_scores", "_look_ahead", "_bind_view", "top_clips"):
        setattr(ticket_cls, name, getattr(TicketScoring, name))
    ticket_cls._review_band = staticmethod(TicketScoring._review_band)
    for name in ("feature_db", "feature_db_dtype", "device", "_round", "_score_weights", "_ahead", "_hp", "_stream_gap", "_view", "_fit", "_fit_round", "_top", "_top_round",
                 "_top_weights"):
        if not hasattr(ticket_cls, name):
            setattr(ticket_cls, name, getattr(TicketScoring, name))
    if hyperparameter_cls is not None:
        from .hyperparameter import Hyperparameter
        for name in ("optimize_weights", "_labelled_rows", "_refine", "_pick", "_pick_from"):
            setattr(hyperparameter_cls, name, Hyperparameter.__dict__[name])
