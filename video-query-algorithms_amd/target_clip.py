"""The query vectors of a round: the seam of the reference's ``TargetClip`` (src/models/target_clip.py) over this
package's own data model.

What ``compute_matches`` and ``Ticket`` read from the object is kept -- ``TargetClip(ticket, hyperparameters)``,
``get_target_features()``, ``target_features`` ({stream: {split: list}}, JSON-serialisable for ticket.py:296),
``splits``, ``previous_target_features`` -- everything behind it is built differently:

* the validated clips of a round are gathered ONCE into a :class:`ValidatedPool`: dense ``[clip][stream][slot][D]``
  blocks with a presence mask (or, when the ticket carries a resident :class:`FeatureDB` that holds the clips, just
  their row numbers -- no feature leaves the device);
* a round is a list of *draws* (index sets into the pool; the calls into ``random`` follow the protocol of
  target_clip.py:297-309 so that a seeded broker picks the same clips), and every (draw, stream, split) problem of
  the round is solved by ONE launch of the closed-form kernel (csrc/vq_boot.hip: Gram matrix + Woodbury instead of
  the 1024 x 1024 inverses of target_clip.py:192-197 / :245-260);
* bagging averages the draws, ``partial_update`` blends with the previous round's target (target_clip.py:75-82);
* a round is PLANNED (REST, draws) and then SOLVED: alone (``get_target_features``), or with the planned rounds of the other tickets
  of a broker pass whose clips are rows of the same resident database (:func:`solve_targets_batch`: one
  ``FeatureDB.batch_targets`` call for up to 16 tickets instead of one call per draw).

SURVEY.md 8(a) row B1 (``t = r / (r . r)`` of the reference clip, target_clip.py:137-143, :263-286, :311-313) is
the no-adjustment case; 8(f) row 1 is the rest.
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .bootstrap import bootstrap_targets

ADJUSTMENTS = ("simple", "partial_update", "bagging")


def clip_vectors(records, streams: Sequence[str], feature_name: str):
    """The API's feature records of one clip (wire format of target_clip.py:279-285) -> ({stream: {split: vector}},
    splits seen).  Records of other streams or other blobs are skipped."""
    table: Dict[str, dict] = {st: {} for st in streams}
    for rec in records:
        per_stream = table.get(rec["dnn_stream_id"])
        if per_stream is not None and rec["name"] == feature_name:
            per_stream[rec["dnn_stream_split"]] = rec["feature_vector"]
    return table, {sp for per_stream in table.values() for sp in per_stream}


def unit_response(vec) -> list:
    """``r / (r . r)``: the vector whose dot product with r is exactly 1 (target_clip.py:311-313)."""
    r = np.asarray(vec, dtype=np.float64)
    return (r / np.dot(r, r)).tolist()


def draw_indices(count: int, fraction, with_replacement: bool) -> List[int]:
    """Which of `count` validated clips enter one problem.  RNG protocol of target_clip.py:297-309: round(count *
    fraction) but at least one; ``random.sample`` without, ``random.choices`` with replacement; duplicates collapse
    through a ``set`` whose iteration order is the row order of the problem."""
    k = max(round(count * fraction), 1)
    population = range(count)
    hits = random.choices(population, k=k) if with_replacement else random.sample(population, k)
    return list(set(hits))


class ValidatedPool:
    """The user-validated clips of one kind (confirmed matches, or confirmed non-matches) of a round."""

    def __init__(self, streams: Sequence[str]):
        self.streams = list(streams)
        self.tables: List[dict] = []        # per clip {stream: {split: vector}} (record-fed)
        self.rows: List[int] = []           # per clip its row in the resident FeatureDB (row-fed)
        self.splits: set = set()

    def __len__(self):
        return len(self.tables) or len(self.rows)

    def add_table(self, table, splits):
        self.tables.append(table)
        self.splits |= set(splits)

    def stack(self, picked: Sequence[int], stream: str, split) -> np.ndarray:
        """[m][D] fp64: the (stream, split) vectors of the picked clips that have one, in pick order."""
        vecs = [self.tables[i][stream][split] for i in picked if split in self.tables[i][stream]]
        return np.asarray(vecs, dtype=np.float64).reshape(len(vecs), -1)


class TargetClip:
    def __init__(self, ticket, hyperparameters):
        self._ticket = ticket
        self.hyperparameters = hyperparameters
        self.client, self.schema = getattr(ticket, "client", None), getattr(ticket, "schema", None)
        self.bootstrap_target = bool(ticket.dynamic_target_adjustment)
        self.latest_query_result = ticket.latest_query_result
        earlier = (self.latest_query_result or {}).get("bootstrapped_target")
        self.previous_target_features = earlier or None
        self.ref_clip_features, self.splits = self._get_clip_features(ticket.ref_clip_id)
        self.target_features: dict = {}
        self._planned = None                 # (kind, valid pool, invalid pool, draws) between plan_target_features and the solve

    # ------------------------------------------------------------------ the seam
    def get_target_features(self):
        """Sets ``self.target_features`` for this round (decision ladder of target_clip.py:26-73): the round is planned, then solved
        on its own.  ``compute_matches(batch_targets=True)`` plans every ticket's target first and solves the planned ones of a group
        in one call (:func:`solve_targets_batch`)."""
        if self.plan_target_features():
            self.solve_planned_target()

    def plan_target_features(self) -> bool:
        """Everything of the round that talks to the API or draws from ``random``, in the order of the reference: the validated
        clips (REST), the check of ``bootstrap_type``, the draws of the adjustment mode.  Without validated matches the target is the
        scaled reference clip and nothing is left to do (False); otherwise the round's problems are kept on the object until
        ``solve_planned_target`` or ``solve_targets_batch`` solves them (True)."""
        self._planned = None
        pools = self._validated_pools() if self.bootstrap_target and self.latest_query_result is not None else None
        if not pools or not len(pools[0]):
            self.target_features = self.scaled_ref_clip_features()
            return False
        hp = self.hyperparameters
        kind = hp.bootstrap_type
        if kind not in ADJUSTMENTS:
            raise Exception("Error: bootstrap_type should be one of 'simple', 'partial_update', or 'bagging'")
        valid, invalid = pools
        if kind == "bagging":
            draws = [self._draw(valid, invalid, 1, True) for _ in range(hp.nbags)]
        else:
            draws = [self._draw(valid, invalid, hp.f_bootstrap, False)]
        self._planned = (kind, valid, invalid, draws)
        return True

    def solve_planned_target(self):
        """The planned round solved on its own: one launch for a record-fed pool, one call per draw on resident rows."""
        kind, valid, invalid, draws = self._planned
        self._planned = None
        self._adopt_solved(kind, valid, self._solve(valid, invalid, draws))

    def scaled_ref_clip_features(self):
        return {st: {sp: unit_response(v) for sp, v in per_split.items()}
                for st, per_split in self.ref_clip_features.items()}

    # ------------------------------------------------------------------ the three adjustment modes
    def _adopt_solved(self, kind, valid, bags):
        """The draws' targets -> ``target_features``: the one draw of ``simple``, the mean of the bags (target_clip.py:64-73), the
        blend with the previous round's target of ``partial_update`` (target_clip.py:75-82)."""
        hp = self.hyperparameters
        if kind == "bagging":
            self.target_features = {st: {sp: np.average([b[st][sp] for b in bags], axis=0).tolist() for sp in valid.splits}
                                    for st in hp.streams}
            return
        self.target_features = bags[0]
        if kind == "partial_update":
            keep = hp.f_memory
            for st, sp, old in self._previous_vectors(valid):
                mine = self.target_features[st]
                mine[sp] = (np.multiply(keep, mine[sp]) + np.multiply((1 - keep), old)).tolist()

    def _previous_vectors(self, valid):
        """(stream, split, the previous round's vector) for every slot a ``partial_update`` round blends, in its order; nothing when
        there is no previous target.  A stream or split the previous target lacks raises KeyError."""
        before = self.previous_target_features
        if not before:
            return
        for st in self.hyperparameters.streams:
            theirs = before[st]
            for sp in valid.splits:
                yield st, sp, (theirs[sp] if sp in theirs else theirs[str(sp)])      # JSON round trips turn keys into strings

    # ------------------------------------------------------------------ draws and the device solve
    @staticmethod
    def _draw(valid, invalid, fraction, with_replacement) -> Tuple[List[int], List[int]]:
        """One problem's clips.  With confirmed non-matches both kinds are always subsampled (target_clip.py:227-230);
        without, the matches are only touched when that changes something (:181-182) -- the generator must advance
        exactly as often as the reference's."""
        if len(invalid):
            return (draw_indices(len(valid), fraction, with_replacement),
                    draw_indices(len(invalid), fraction, with_replacement))
        if fraction != 1 or with_replacement:
            return draw_indices(len(valid), fraction, with_replacement), []
        return list(range(len(valid))), []

    def _solve(self, valid, invalid, draws) -> List[dict]:
        """All (draw, stream, split) problems of the round in one launch -> per draw {stream: {split: list}}."""
        hp = self.hyperparameters
        device = getattr(self._host(), "device", 0) or 0
        if valid.rows:
            return [self._solve_resident(valid, invalid, d) for d in draws]
        slots = [(st, sp) for st in hp.streams for sp in valid.splits]
        problems = []
        for picked_valid, picked_invalid in draws:
            for st, sp in slots:
                problems.append((valid.stack(picked_valid, st, sp),
                                 invalid.stack(picked_invalid, st, sp) if picked_invalid else None))
        solved = iter(bootstrap_targets(problems, hp.mu, device=device))
        out = []
        for _ in draws:
            target = {st: {} for st in hp.streams}
            for st, sp in slots:
                target[st][sp] = next(solved).tolist()
            out.append(target)
        return out

    def _solve_resident(self, valid, invalid, draw) -> dict:
        """The clips live in the ticket's FeatureDB: the kernel reads their rows in place."""
        db = self._host().feature_db
        picked_valid, picked_invalid = draw
        t = db.bootstrap_target([valid.rows[i] for i in picked_valid], [invalid.rows[i] for i in picked_invalid],
                                mu=self.hyperparameters.mu, set_query=False)
        return {st: {sp: t[db.stream_names.index(st), e].tolist() for e, sp in enumerate(db.slot_splits[db.stream_names.index(st)])}
                for st in self.hyperparameters.streams}

    # ------------------------------------------------------------------ gathering the validated clips
    def _validated_pools(self) -> Optional[Tuple[ValidatedPool, ValidatedPool]]:
        verdicts = self._match_verdicts()
        hp = self.hyperparameters
        valid, invalid = ValidatedPool(hp.streams), ValidatedPool(hp.streams)
        db = getattr(self._host(), "feature_db", None)
        clips = [c for c, _ in verdicts]
        if db is not None and self._resident_ok(db, clips):
            for clip, verdict in verdicts:
                (valid if verdict else invalid).rows.append(db.row_of(clip))
            valid.splits = set(db.slot_splits[0])
            return valid, invalid
        for clip, verdict in verdicts:
            (valid if verdict else invalid).add_table(*self._get_clip_features(clip))
        return valid, invalid

    def _resident_ok(self, db, clips) -> bool:
        """Rows can be used in place when the DB knows its slot layout, is dense, carries every stream of the round
        with one common split list, and holds every validated clip."""
        names, slots = getattr(db, "stream_names", None), getattr(db, "slot_splits", None)
        if not names or not slots or db.present is not None:
            return False
        if any(st not in names for st in self.hyperparameters.streams) or any(s != slots[0] for s in slots):
            return False
        return bool(clips) and all(db.has_clip(c) for c in clips)

    def _match_verdicts(self) -> List[Tuple[int, bool]]:
        """(clip id, user verdict) of every match of the latest query result the user has judged, in the API's order
        (all pages of ["matches", "list"], target_clip.py:117-124)."""
        judged, page = [], 1
        while page is not None:
            answer = self._request(["matches", "list"], {"query_result": self.latest_query_result["id"], "page": page})
            judged += [(m["video_clip"], m["user_match"]) for m in answer["results"]
                       if m["user_match"] is True or m["user_match"] is False]
            page = answer["pagination"]["nextPage"]
        return judged

    def _get_clip_features(self, clip_id):
        hp = self.hyperparameters
        return clip_vectors(self._request(["video-clips", "features"], {"id": clip_id}), hp.streams, hp.feature_name)

    def _host(self):
        """The ticket this target belongs to (None on a reference-class instance that install() did not wrap)."""
        return getattr(self, "_ticket", None)

    def _request(self, action, params):
        return self._ticket._request(action, params)


# what install() grafts onto the reference's TargetClip: the round logic; its own __init__ (wrapped to remember the
# ticket), _get_clip_features and _request (REST) stay the reference's
GRAFTED = ("get_target_features", "plan_target_features", "solve_planned_target", "scaled_ref_clip_features", "_adopt_solved",
           "_previous_vectors", "_draw", "_solve", "_solve_resident", "_validated_pools", "_resident_ok", "_match_verdicts", "_host")


def _batch_entry(target):
    """What ``FeatureDB.batch_targets`` needs of a planned, row-fed target: (pool, draws, mu, previous [S,E,D] or None, keep)."""
    kind, valid, invalid, draws = target._planned
    hp, db = target.hyperparameters, target._host().feature_db
    previous = None
    if kind == "partial_update":
        blended = list(target._previous_vectors(valid))
        if blended:
            previous = np.zeros((db.S, db.E, db.D), dtype=np.float64)
            for st, sp, old in blended:
                s = db.stream_names.index(st)
                previous[s, db.slot_splits[s].index(sp)] = old
    return (valid.rows, invalid.rows), draws, hp.mu, previous, hp.f_memory


def _adopt_batched(target, t):
    """``t`` [S,E,D] of ``batch_targets`` -> the nested dict of lists a solve of the target's own leaves, key order included."""
    kind, valid, _invalid, _draws = target._planned
    target._planned = None
    db = target._host().feature_db
    hp = target.hyperparameters
    index = {st: db.stream_names.index(st) for st in hp.streams}
    if kind == "bagging":
        target.target_features = {st: {sp: t[index[st], db.slot_splits[index[st]].index(sp)].tolist() for sp in valid.splits} for st in hp.streams}
    else:
        target.target_features = {st: {sp: t[index[st], e].tolist() for e, sp in enumerate(db.slot_splits[index[st]])} for st in hp.streams}


def _batchable_db(target):
    """The database whose ``batch_targets`` can solve this target with others: it is planned, its pools are rows of the ticket's
    resident database, and that database has the call (a ShardedFeatureDB and the numpy stand-ins of the tests do not)."""
    planned = getattr(target, "_planned", None)
    if planned is None or not planned[1].rows:
        return None
    db = getattr(target._host(), "feature_db", None)
    return db if callable(getattr(db, "batch_targets", None)) else None


def solve_targets_batch(targets):
    """Solves the planned targets of a broker pass (``plan_target_features`` returned True; the others are skipped).  Targets whose
    pools are rows of the SAME resident ``FeatureDB`` object share calls of ``FeatureDB.batch_targets`` -- at most 16 per call, in
    list order, a call as soon as it is full, under the database's lock: every draw of every such ticket in one call instead of one
    call per draw.  Every other target -- a record-fed pool, a database without the call, the only one of its database -- solves on
    its own as in ``get_target_features``, in list order.  ``target_features`` is what the target's own solve leaves, bit for bit.  A
    singular system raises ``VqError`` as the one-draw call does; a missing key of ``previous_target_features`` raises its KeyError."""
    from .ticket import _db_lock
    waiting: Dict[int, list] = {}

    def flush(group):
        if len(group) == 1:
            group[0].solve_planned_target()
            return
        db = group[0]._host().feature_db
        entries = [_batch_entry(t) for t in group]
        with _db_lock(db):
            solved = db.batch_targets([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries],
                                      previous=[e[3] for e in entries], keeps=[e[4] for e in entries])
        for t, arr in zip(group, solved):
            _adopt_batched(t, arr)

    for target in targets:
        if getattr(target, "_planned", None) is None:
            continue
        db = _batchable_db(target)
        if db is None:
            target.solve_planned_target()
            continue
        group = waiting.setdefault(id(db), [])
        group.append(target)
        if len(group) == 16:
            flush(waiting.pop(id(db)))
    for group in waiting.values():
        flush(group)
