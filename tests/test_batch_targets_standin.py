"""CPU: compute_matches(batch=True, batch_targets=True) and target_clip.solve_targets_batch on the numpy stand-in database
(tests/_standin_targets.py) -- which tickets get their target bootstrapping in the group's call, which calls that leaves, and that the
run is the batch=True run value for value: ledger, draws from ``random``, target_features, matches (the stand-in is the same numpy
either way; the device side is covered by tests/test_batch_targets_gpu.py)."""
import random

import pytest

import bootstrap_oracle as bo
import numpy as np

from _helpers import DEFAULT_WEIGHTS, SEED, STREAMS, records_from_dense
from _standin_targets import BootOracleFeatureDB, TargetsOracleFeatureDB
from test_batch_tickets_standin import IDS, X, _db, _labelled, _Repo, _update

import video_query_algorithms_amd as vqa

LATER = {"latest_query_result": {"round": 1, "bootstrapped_target": None, "id": 3}}
HOST_ROUTE = []       # the problems of every launch through the host-row route (a record-fed pool)


@pytest.fixture(autouse=True)
def host_route_on_the_oracle(monkeypatch):
    """There is no device here: the one launch of a record-fed pool (bootstrap.bootstrap_targets) is the oracle's restatement too."""
    def solve(problems, mu, device=0):
        HOST_ROUTE.append(len(problems))
        return [bo.kernel_order_target(X, Y, mu)[0] for X, Y in problems]
    del HOST_ROUTE[:]
    monkeypatch.setattr(vqa.target_clip, "bootstrap_targets", solve)


def _hp(kind="bagging", f_bootstrap=1):
    return vqa.Hyperparameter(DEFAULT_WEIGHTS, 0.8, 0.0, 0.35, 0.3, STREAMS, "global_pool", f_bootstrap, 0.7, kind, 3)


def _revise(db, row, adjust=True, masked=False, verdicts=None, **kw):
    """A revise update on clip ``row`` whose user judged the first round's matches; ``verdicts`` rewrites the judged list.  ``masked``:
    the ticket gets a database of its own with a presence mask, which sends its validated clips down the record path -- their API
    records then travel with the update."""
    matches, user = _labelled(db, row)
    listed = [{"video_clip": m["video_clip"], "user_match": m["user_match"]} for m in matches]
    if verdicts is not None:
        listed = verdicts(listed)
    more = dict(LATER, feature_db=db, **kw)
    if masked:
        present = np.ones(X.shape[:3], dtype=bool)
        present[-1, 0, 0] = False
        more["feature_db"] = type(db)(X, present=present, stream_names=list(STREAMS), slot_splits=[[1, 2, 3]] * 2, clip_ids=IDS)
        rows = sorted({row} | {more["feature_db"].row_of(m["video_clip"]) for m in listed})
        more["records"] = records_from_dense(X[rows], IDS[rows], [1, 2, 3])
    return ("revise", _update(row, matches=matches, user_matches=user, dynamic_target_adjustment=adjust, match_list=listed, **more))


def _run(pairs_for, cls, hp=None, **kw):
    """compute_matches over ``pairs_for(db)`` on a fresh stand-in of class ``cls`` -> (db, tickets, hp, the next random number)."""
    db = _db(cls)
    pairs = pairs_for(db)
    made = []
    real_init = vqa.Ticket.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    vqa.Ticket.__init__ = spy
    hp = hp or _hp()
    try:
        db.log.clear()
        random.seed(a=SEED)
        vqa.compute_matches(_Repo(pairs), hp, **kw)
    finally:
        vqa.Ticket.__init__ = real_init
    return db, made, hp, random.random()


def _outcome(made, hp, after):
    return ([tk.ledger for tk in made], [tk.target.target_features for tk in made],
            [list(tk.matches.items()) if isinstance(tk.matches, dict) else tk.matches for tk in made], dict(hp.weights), hp.threshold, after)


def _calls(db, kind):
    return [x for k, x in db.log if k == kind]


def _mixed(db):
    nobody = lambda listed: [dict(m, user_match=None) for m in listed]                       # noqa: E731
    return [("new", _update(5, feature_db=db)),                                              # a new query: the scaled reference clip
            _revise(db, 60), _revise(db, 90),                                                # eligible
            _revise(db, 120, masked=True),                                                   # record-fed pool (a database with a presence mask)
            _revise(db, 150, verdicts=nobody),                                               # no validated match: adjustment switched off
            _revise(db, 180, adjust=False),                                                  # no bootstrapping
            ("new", None), _revise(db, 210)]                                                 # eligible


@pytest.mark.parametrize("kind", ["bagging", "simple", "partial_update"])
def test_the_group_solve_equals_the_per_ticket_solves(kind):
    def pairs(db):
        out = _mixed(db)
        if kind == "partial_update":                                                         # one of the eligible tickets has a previous target
            prev = {st: {str(sp): [0.25 * (sp + i % 7) for i in range(db.D)] for sp in (1, 2, 3)} for st in STREAMS}
            out[2][1]["latest_query_result"] = dict(LATER["latest_query_result"], bootstrapped_target=prev)
        return out
    got = _run(pairs, TargetsOracleFeatureDB, hp=_hp(kind, 0.5), batch=True, batch_targets=True)
    want = _run(pairs, TargetsOracleFeatureDB, hp=_hp(kind, 0.5), batch=True)
    assert len(got[1]) == len(want[1]) == 7
    assert _outcome(*got[1:]) == _outcome(*want[1:])
    # the three eligible tickets share ONE call; only the record-fed one solves alone (one launch through the host-row route: no "boot")
    assert len(_calls(got[0], "targets")) == 1 and len(_calls(got[0], "targets")[0]) == 3 and not _calls(got[0], "boot")
    assert not _calls(want[0], "targets") and len(_calls(want[0], "boot")) == 3 * (3 if kind == "bagging" else 1)
    assert HOST_ROUTE == [6 * (3 if kind == "bagging" else 1)] * 2                           # the record-fed ticket, once per run
    assert all(tk.target._planned is None for tk in got[1])
    assert got[1][2].target.target_features != got[1][2].target.scaled_ref_clip_features()


def test_seventeen_eligible_tickets_make_two_calls():
    rows = list(range(10, 10 + 17 * 9, 9))

    def pairs(db):
        return [_revise(db, r) for r in rows]
    got = _run(pairs, TargetsOracleFeatureDB, batch=True, batch_targets=True)
    want = _run(pairs, TargetsOracleFeatureDB, batch=True)
    assert [len(x) for x in _calls(got[0], "targets")] == [16]                               # 16 in the group's call ...
    assert len(_calls(got[0], "boot")) == 3                                                  # ... the lone one on its own path: a call per bag
    assert _outcome(*got[1:]) == _outcome(*want[1:])
    assert int(IDS[rows[16]]) in got[1][16].matches


def test_a_database_without_the_method_and_a_group_of_one_solve_alone():
    got = _run(_mixed, BootOracleFeatureDB, batch=True, batch_targets=True)
    want = _run(_mixed, BootOracleFeatureDB, batch=True)
    assert _calls(got[0], "boot") == _calls(want[0], "boot") and len(_calls(got[0], "boot")) == 9
    assert _outcome(*got[1:]) == _outcome(*want[1:])
    one = _run(lambda db: [_revise(db, 60), ("new", _update(5, feature_db=db))], TargetsOracleFeatureDB, batch=True, batch_targets=True)
    ref = _run(lambda db: [_revise(db, 60), ("new", _update(5, feature_db=db))], TargetsOracleFeatureDB, batch=True)
    assert not _calls(one[0], "targets") and len(_calls(one[0], "boot")) == 3
    assert _outcome(*one[1:]) == _outcome(*ref[1:])


def test_a_custom_target_class_without_the_planning_method_is_left_alone():
    class Plain:
        def __init__(self, ticket, hp):
            self._inner = vqa.TargetClip(ticket, hp)
            self.previous_target_features = self._inner.previous_target_features

        def get_target_features(self):
            self._inner.get_target_features()
            self.target_features, self.splits = self._inner.target_features, self._inner.splits

        _planned = None
    pairs = lambda db: [_revise(db, 60), _revise(db, 90)]                                    # noqa: E731
    got = _run(pairs, TargetsOracleFeatureDB, batch=True, batch_targets=True, target_factory=Plain)
    want = _run(pairs, TargetsOracleFeatureDB, batch=True, target_factory=Plain)
    assert not _calls(got[0], "targets") and len(_calls(got[0], "boot")) == 6
    assert _outcome(*got[1:]) == _outcome(*want[1:])


def test_batch_targets_needs_batch():
    with pytest.raises(ValueError):
        vqa.compute_matches(_Repo([]), _hp(), batch_targets=True)


def test_a_status_on_query_k_raises_for_ticket_k():
    twice = lambda listed: listed + [m for m in listed if m["user_match"] is True][:1]       # noqa: E731  a clip validated twice: dependent rows

    def pairs(db):
        return [_revise(db, 60), _revise(db, 90, verdicts=twice), _revise(db, 210)]
    hp = _hp("simple", 1)                                                                    # every draw is its whole pool
    with pytest.raises(vqa.VqError) as group:
        _run(pairs, TargetsOracleFeatureDB, hp=hp, batch=True, batch_targets=True)
    assert group.value.code == -1 and "query 1," in str(group.value) and "singular system" in str(group.value)
    with pytest.raises(vqa.VqError) as alone:
        _run(pairs, TargetsOracleFeatureDB, hp=_hp("simple", 1), batch=True)
    assert alone.value.code == -1 and "singular system" in str(alone.value)


def test_an_unknown_bootstrap_type_and_a_missing_previous_key_raise_as_ever():
    for kw in ({"batch": True}, {"batch": True, "batch_targets": True}):
        with pytest.raises(Exception, match="bootstrap_type should be one of"):
            _run(lambda db: [_revise(db, 60), _revise(db, 90)], TargetsOracleFeatureDB, hp=_hp("bogus"), **kw)

        def pairs(db):
            out = [_revise(db, 60), _revise(db, 90)]
            prev = {"rgb": {str(sp): [1.0] * db.D for sp in (1, 2, 3)}}                      # the second stream is missing
            out[1][1]["latest_query_result"] = dict(LATER["latest_query_result"], bootstrapped_target=prev)
            return out
        with pytest.raises(KeyError):
            _run(pairs, TargetsOracleFeatureDB, hp=_hp("partial_update", 0.5), **kw)
