"""CPU: compute_matches(batch=True, fit_weights=True) and ticket.compute_similarities_batch(fit=...) on the numpy stand-in database --
which tickets get their weight update behind the group's pass, which calls that leaves, and that the run is the batch=True run
value for value (the stand-in is the same numpy either way; the device side is covered by tests/test_batch_fit_gpu.py and
tests/test_batch_fit_tickets_gpu.py)."""
import random

import numpy as np
import pytest

import sim_oracle as so
from _helpers import SEED
from _search_set_cases import host_loss_surface, np_select
from test_batch_tickets_standin import IDS, RoundOracleFeatureDB, _db, _hp, _labelled, _Repo, _ticket, _update

import video_query_algorithms_amd as vqa
from video_query_algorithms_amd.feature_db import RoundResult

LATER = {"latest_query_result": {"round": 1, "bootstrapped_target": None, "id": 3}}


class FitOracleFeatureDB(RoundOracleFeatureDB):
    """RoundOracleFeatureDB plus FeatureDB.batch_round_fit / batch_round_rescore in numpy, over the avg the last batched call kept;
    ``log`` also records the one-query calls a weight update makes."""

    def query_round_batch(self, targets, weights, selects=None, want_avg=True):
        out = super().query_round_batch(targets, weights, selects, want_avg)
        self._kept = [(r.avg, r.n_e) for r in out]
        return out

    def query_round(self, t, weights=None, select=None):
        if t is None:
            self.log.append(("round", []))
        return super().query_round(t, weights, select)

    def write_avg(self, avg, n_e=None):
        self.log.append(("write_avg", []))
        super().write_avg(avg, n_e)

    def scores_grid(self, w_grid, rows):
        self.log.append(("scores_grid", []))
        return super().scores_grid(w_grid, rows)

    def select(self, threshold, lower):
        self.log.append(("select", []))
        return super().select(threshold, lower)

    def batch_round_fit(self, queries, rows, labels, w_grids, th_grids, ballasts):
        self.log.append(("fit", list(queries)))
        out = []
        for q, r, y, wg, th, ballast in zip(queries, rows, labels, w_grids, th_grids, ballasts):
            avg = self._kept[q][0]
            graded = np.stack([so.dense_scores(avg[np.asarray(r, dtype=np.int64)], w) for w in np.asarray(wg)])
            out.append(host_loss_surface(graded, y, th, ballast))
        return out

    def batch_round_rescore(self, queries, weights, selects=None):
        self.log.append(("rescore", list(queries)))
        out = []
        for i, q in enumerate(queries):
            r = RoundResult()
            r.avg, r.n_e = self._kept[q]
            r.scores = so.dense_scores(r.avg, weights[i])
            r.match_rows = r.near_rows = None
            r.near_argmax = -1
            if selects is not None:
                r.match_rows, r.near_rows, r.near_argmax = np_select(r.scores, float(selects[i][0]), float(selects[i][1]))
            out.append(r)
        return out


def _kinds(db, *names):
    return [kind for kind, _ in db.log if kind in names]


def _run(pairs_for, cls, **kw):
    """compute_matches over ``pairs_for(db)`` on a fresh stand-in of class ``cls`` -> (db, tickets, hp)."""
    db = _db(cls)
    pairs = pairs_for(db)
    made = []
    real_init = vqa.Ticket.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    vqa.Ticket.__init__ = spy
    hp = _hp()
    try:
        db.log.clear()
        random.seed(a=SEED)
        vqa.compute_matches(_Repo(pairs), hp, **kw)
    finally:
        vqa.Ticket.__init__ = real_init
    return db, made, hp


def _outcome(made, hp):
    return ([tk.ledger for tk in made], [list(tk.matches.items()) if isinstance(tk.matches, dict) else tk.matches for tk in made],
            dict(hp.weights), hp.threshold)


def _revise(db, row, kind="revise"):
    matches, user = _labelled(db, row)
    return (kind, _update(row, feature_db=db, matches=matches, user_matches=user, **LATER))


def _mixed(db):
    return [("new", _update(5, feature_db=db)), ("new", _update(70, feature_db=db)), ("new", None), _revise(db, 60),
            ("new", _update(120, feature_db=db, ref_clip_id=None)),                          # fatal in phase 1: never scanned
            _revise(db, 60, "finalize"), ("new", _update(130, feature_db=db)), _revise(db, 90), _revise(db, 150)]


def test_fitted_pass_equals_the_batched_pass_and_makes_two_calls():
    db_f, made_f, hp_f = _run(_mixed, FitOracleFeatureDB, batch=True, fit_weights=True)
    db_b, made_b, hp_b = _run(_mixed, FitOracleFeatureDB, batch=True)
    assert len(made_f) == len(made_b) == 8
    assert [tk.ledger["process_state"] for tk in made_f] == [[3, 4], [3, 4], [3, 4], [3, 5], [3, 7], [3, 4], [3, 4], [3, 4]]
    assert _outcome(made_f, hp_f) == _outcome(made_b, hp_b)
    # one pass, one fit and one rescore for the three revise tickets and the finalize one (slots 2, 3, 5, 6 of the seven in the pass)
    assert _kinds(db_f, "batch", "fit", "rescore", "scan") == ["batch", "fit", "rescore"]
    assert [qs for kind, qs in db_f.log if kind in ("fit", "rescore")] == [[2, 3, 5, 6]] * 2
    # the finalize ticket's own band: its similarities go back once and it selects once, as on the parent; nothing else is asked
    assert _kinds(db_f, "write_avg", "select", "scores_grid", "round") == ["write_avg", "select"]
    assert _kinds(db_b, "write_avg", "scores_grid", "round").count("scores_grid") == 4 and _kinds(db_b, "write_avg").count("write_avg") == 4
    assert not _kinds(db_b, "fit", "rescore")
    for tk in made_f:
        assert (tk._fit is not None) == (tk.query_id in (60, 90, 150))


def test_a_ticket_alone_in_its_group_fits_on_its_own():
    db, made, hp = _run(lambda d: [_revise(d, 60)], FitOracleFeatureDB, batch=True, fit_weights=True)
    ref_db, ref_made, ref_hp = _run(lambda d: [_revise(d, 60)], FitOracleFeatureDB, batch=True)
    assert _kinds(db, "batch", "fit", "rescore", "scan", "scores_grid") == ["scan", "scores_grid"] and made[0]._fit is None
    assert _outcome(made, hp) == _outcome(ref_made, ref_hp)


def test_a_database_without_the_two_methods_falls_back():
    db, made, hp = _run(_mixed, RoundOracleFeatureDB, batch=True, fit_weights=True)
    ref_db, ref_made, ref_hp = _run(_mixed, RoundOracleFeatureDB, batch=True)
    assert _kinds(db, "batch", "scan") == ["batch"] and all(tk._fit is None for tk in made)
    assert _outcome(made, hp) == _outcome(ref_made, ref_hp)


def test_a_member_without_labels_is_left_to_optimize_weights():
    hp = _hp()
    db = _db(FitOracleFeatureDB)
    matches, user = _labelled(db, 60)
    tickets = [_ticket(db, 60, hp, matches=matches, user_matches=user), _ticket(db, 90, hp, matches=[]), _ticket(db, 5, hp)]
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, True, False])
    assert [(kind, qs) for kind, qs in db.log if kind in ("fit", "rescore")] == [("fit", [0]), ("rescore", [0])]
    assert tickets[0]._fit is not None and tickets[0]._fit_round is tickets[0]._round and tickets[1]._fit is None and tickets[2]._fit is None
    weights, th = tickets[0]._fit
    assert tickets[0]._ahead["select"] == (float(th), float(th) - hp.near_miss_default * (1 - float(th)))
    # nobody labelled: no call at all
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets[1:], hp, fit=[True, True])
    assert _kinds(db, "batch", "fit", "rescore") == ["batch"]
    # a later round of the ticket's own drops the fit: its _round token changed
    tickets[0].compute_similarities(hp)
    assert tickets[0]._fit_round is not tickets[0]._round
    with pytest.raises(ValueError):
        vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True])


def test_more_than_sixteen_tickets_fit_behind_their_own_pass():
    rows = list(range(10, 10 + 17 * 9, 9))                                                   # 17 revise tickets and a new one: passes of 16 and 2

    def pairs(db):
        return [_revise(db, r) for r in rows] + [("new", _update(200, feature_db=db))]
    db_f, made_f, hp_f = _run(pairs, FitOracleFeatureDB, batch=True, fit_weights=True)
    db_b, made_b, hp_b = _run(pairs, FitOracleFeatureDB, batch=True)
    assert [(kind, len(x)) for kind, x in db_f.log if kind in ("batch", "fit", "rescore")] == \
        [("batch", 16), ("fit", 16), ("rescore", 16), ("batch", 2), ("fit", 1), ("rescore", 1)]
    assert not _kinds(db_f, "write_avg", "scores_grid", "select", "round", "scan")
    assert _outcome(made_f, hp_f) == _outcome(made_b, hp_b)
    assert int(IDS[rows[16]]) in made_f[16].matches


def test_fit_weights_needs_batch():
    with pytest.raises(ValueError):
        vqa.compute_matches(_Repo([]), _hp(), fit_weights=True)
