"""CPU: ticket.compute_similarities_batch(top=...), TicketScoring.top_clips and compute_matches(batch=True, top=...) on a numpy stand-in
database -- who gets a ranking, from which call, in which order behind the pass and the fit, and when top_clips may serve it (the
device side of the ranking is covered by tests/test_batch_topk_gpu.py)."""
import numpy as np
import pytest

from _helpers import DEFAULT_WEIGHTS
from _search_set_cases import np_topk, same_bits
from test_batch_fit_standin import FitOracleFeatureDB, _kinds, _revise, _run
from test_batch_tickets_standin import IDS, _db, _hp, _labelled, _Repo, _ticket, _update

import video_query_algorithms_amd as vqa


class TopOracleFeatureDB(FitOracleFeatureDB):
    """FitOracleFeatureDB plus FeatureDB.batch_round_topk in numpy, over the scores the last batched call -- or the rescore behind it --
    left; ``log`` also records the one-query ``topk`` calls."""

    def query_round_batch(self, targets, weights, selects=None, want_avg=True):
        out = super().query_round_batch(targets, weights, selects, want_avg)
        self._left = [np.array(r.scores) for r in out]
        return out

    def batch_round_rescore(self, queries, weights, selects=None):
        out = super().batch_round_rescore(queries, weights, selects)
        for q, r in zip(queries, out):
            self._left[q] = np.array(r.scores)
        return out

    def batch_round_topk(self, ks, queries=None):
        queries = list(range(len(self._left))) if queries is None else list(queries)
        ks = [int(ks)] * len(queries) if np.ndim(ks) == 0 else [int(k) for k in ks]
        self.log.append(("btopk", ks))
        return [np_topk(self._left[q], k) for q, k in zip(queries, ks)]

    def topk(self, k):
        self.log.append(("topk", [k]))
        return np_topk(self._scores, k)


def _expect(tk, k):
    rows, vals = np_topk(np.asarray(tk._ahead["scores"]), k)
    return tk._view.clip_ids[rows], vals


def _same_top(got, want):
    return np.array_equal(got[0], want[0]) and same_bits(np.array(got[1]), np.array(want[1]))


def test_every_member_of_a_pass_is_ranked_in_one_call():
    hp, db = _hp(), _db(TopOracleFeatureDB)
    tickets = [_ticket(db, row, hp) for row in (5, 70, 130)]
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp, top=5)
    assert _kinds(db, "batch", "btopk", "topk", "scan") == ["batch", "btopk"] and db.log[-1] == ("btopk", [5, 5, 5])
    for tk in tickets:
        assert tk._top_round is tk._round and len(tk._top) == 2 and len(tk._top[0]) == 5
        assert _same_top(tk._top, _expect(tk, 5))
        assert set(tk._top[0].tolist()) <= set(IDS.tolist()) and tk._top[0][0] == tk.ref_clip_id       # the reference clip is its own best match
    # one k per ticket
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp, top=[1, 7, 300])
    assert db.log[-1] == ("btopk", [1, 7, 300])
    assert [len(tk._top[0]) for tk in tickets] == [1, 7, 300] and all(_same_top(tk._top, _expect(tk, k)) for tk, k in zip(tickets, (1, 7, 300)))
    for bad in ([5, 5], 0, [5, 5, -1]):
        with pytest.raises(ValueError):
            vqa.ticket.compute_similarities_batch(tickets, hp, top=bad)


def test_a_fit_member_is_ranked_under_its_fitted_weights():
    hp, db = _hp(), _db(TopOracleFeatureDB)
    matches, user = _labelled(db, 60)
    tickets = [_ticket(db, 60, hp, matches=matches, user_matches=user), _ticket(db, 5, hp)]
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, False], top=5)
    assert _kinds(db, "batch", "fit", "rescore", "btopk") == ["batch", "fit", "rescore", "btopk"]      # the ranking comes BEHIND the fit
    fitted, plain = tickets
    weights, _th = fitted._fit
    w = np.array([weights[st] for st in fitted._stream_names])
    assert fitted._ahead["w"] == w.tobytes() and fitted._top_weights == w.tobytes()
    assert _same_top(fitted._top, _expect(fitted, 5)) and _same_top(plain._top, _expect(plain, 5))
    fitted.compute_scores(weights)
    db.log.clear()
    assert _same_top(fitted.top_clips(5), fitted._top) and not db.log


def test_a_ticket_alone_in_its_group_gets_the_same_from_topk():
    hp, db = _hp(), _db(TopOracleFeatureDB)
    tk = _ticket(db, 70, hp)
    db.log.clear()
    vqa.ticket.compute_similarities_batch([tk], hp, top=5)
    assert _kinds(db, "batch", "btopk", "scan", "topk") == ["scan", "topk"]
    assert tk._top_round is tk._round and _same_top(tk._top, _expect(tk, 5))


def test_top_clips_serves_the_ranking_or_falls_back():
    hp, db = _hp(), _db(TopOracleFeatureDB)
    tickets = [_ticket(db, row, hp) for row in (5, 70)]
    vqa.ticket.compute_similarities_batch(tickets, hp, top=5)
    tk = tickets[1]
    tk.compute_scores(DEFAULT_WEIGHTS)                                      # the looked-ahead weights: nothing is asked
    db.log.clear()
    ids, vals = tk.top_clips(3)
    assert not db.log                                                       # the database is asked for nothing
    assert np.array_equal(ids, tk._top[0][:3]) and same_bits(np.array(vals), np.array(tk._top[1][:3]))
    # more than the ranking holds: the database ranks the ticket's own scores
    ids, vals = tk.top_clips(9)
    assert _kinds(db, "topk", "btopk") == ["topk"]
    rows, want = np_topk(np.asarray(tk._score_values), 9)
    assert np.array_equal(ids, tk._view.clip_ids[rows]) and same_bits(np.array(vals), want)
    # other weights: the ranking no longer stands for the ticket's scores
    tk.compute_scores({st: w * (2.0 if i else 1.0) for i, (st, w) in enumerate(DEFAULT_WEIGHTS.items())})
    db.log.clear()
    ids, vals = tk.top_clips(3)
    assert _kinds(db, "topk", "btopk") == ["topk"]
    rows, want = np_topk(np.asarray(tk._score_values), 3)
    assert np.array_equal(ids, tk._view.clip_ids[rows]) and same_bits(np.array(vals), want)
    # a later round of the ticket's own: the ranking belongs to the round before
    tk.compute_similarities(hp)
    assert tk._top_round is not tk._round
    tk.compute_scores(DEFAULT_WEIGHTS)
    db.log.clear()
    tk.top_clips(3)
    assert _kinds(db, "topk") == ["topk"]


def test_without_top_nobody_is_ranked():
    hp, db = _hp(), _db(TopOracleFeatureDB)
    tickets = [_ticket(db, row, hp) for row in (5, 70, 130)]
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp)
    assert _kinds(db, "batch", "btopk", "topk") == ["batch"]
    assert all(tk._top is None and tk._top_round is None for tk in tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp, top=4)
    vqa.ticket.compute_similarities_batch(tickets, hp)                        # top=None again: the old ranking is of the round before
    assert all(tk._top_round is not tk._round for tk in tickets)


def test_a_database_without_the_call_ranks_nobody():
    hp, db = _hp(), _db(FitOracleFeatureDB)
    tickets = [_ticket(db, row, hp) for row in (5, 70)]
    vqa.ticket.compute_similarities_batch(tickets, hp, top=5)
    assert all(tk._top is None for tk in tickets)


def test_compute_matches_passes_top_through():
    def pairs(db):
        return [("new", _update(5, feature_db=db)), ("new", _update(70, feature_db=db)), _revise(db, 60)]
    db, made, hp = _run(pairs, TopOracleFeatureDB, batch=True, fit_weights=True, top=5)
    ref_db, ref_made, ref_hp = _run(pairs, TopOracleFeatureDB, batch=True, fit_weights=True)
    assert _kinds(db, "batch", "fit", "rescore", "btopk") == ["batch", "fit", "rescore", "btopk"] and not _kinds(ref_db, "btopk", "topk")
    assert [list(a.matches.items()) for a in made] == [list(b.matches.items()) for b in ref_made] and hp.weights == ref_hp.weights
    assert all(tk._top is not None and len(tk._top[0]) == 5 for tk in made) and all(tk._top is None for tk in ref_made)
    with pytest.raises(ValueError):
        vqa.compute_matches(_Repo([]), _hp(), top=5)


def test_install_grafts_top_clips_and_its_defaults():
    cls = type("Ticket", (), {})
    vqa.install(cls)
    assert cls.top_clips is vqa.TicketScoring.top_clips
    assert cls._top is None and cls._top_round is None
