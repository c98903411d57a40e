"""GPU: tickets with search sets sharing a pass over a resident FeatureDB -- ticket.compute_similarities_batch(..., share_search_sets=True)
and compute_matches(batch=True, share_search_sets=True) against the one-ticket-at-a-time path on a second, identical database."""
import random

import numpy as np
import pytest

import test_batch_tickets_gpu as base
from test_batch_tickets_gpu import REFS, Repo, _prepared, compare_runs, labelled, make_hp, resident, update, vqa  # noqa: F401 -- vqa: the fixture
from _helpers import DEFAULT_WEIGHTS, SEED

pytestmark = pytest.mark.gpu
TOL = 1e-12
SET_ROWS = np.arange(100, 1500, 3)


def test_search_set_tickets_share_one_pass_inside_a_mixed_list(vqa):
    """The mixed list of tests/test_batch_tickets_gpu.py with two more tickets on set 9: the three whole-database tickets and the three
    on set 9 run ONE query_round_batch_sets (3 x 467 + 3 x 2000 >= 2 x 2000), the ticket with another slot mask its own round; every
    ticket equals its solo run (<= 1e-12; n_e, lists and near_argmax exactly, no solo score being within 1e-9 of its band); and a
    search-set ticket that then asks for scores under other weights gets exactly query_round(None, w, band) under its set."""
    from video_query_algorithms_amd.ticket import compute_similarities_batch
    hp = make_hp(vqa)
    hp.weights, hp.threshold = dict(DEFAULT_WEIGHTS), 0.8
    out = []
    for shared in (True, False):
        db = resident(vqa)
        db.define_search_rows(9, SET_ROWS)
        tickets = [_prepared(vqa, db, REFS[0], hp), _prepared(vqa, db, REFS[1], hp, search_set=9), _prepared(vqa, db, REFS[2], hp),
                   _prepared(vqa, db, REFS[3], hp, drop=("rgb", 2)), _prepared(vqa, db, REFS[4], hp),
                   _prepared(vqa, db, 502, hp, search_set=9), _prepared(vqa, db, 904, hp, search_set=9)]
        calls = []
        real_sets, real_batch = type(db).query_round_batch_sets, type(db).query_round_batch

        def spy_sets(self, targets, weights, set_ids, *a, _real=real_sets, **kw):
            calls.append(("sets", list(set_ids)))
            return _real(self, targets, weights, set_ids, *a, **kw)

        def spy_batch(self, targets, *a, _real=real_batch, **kw):
            calls.append(("batch", len(targets)))
            return _real(self, targets, *a, **kw)
        type(db).query_round_batch_sets, type(db).query_round_batch = spy_sets, spy_batch
        try:
            if shared:
                compute_similarities_batch(tickets, hp, share_search_sets=True)
            else:
                for tk in tickets:
                    tk.compute_similarities(hp)
        finally:
            type(db).query_round_batch_sets, type(db).query_round_batch = real_sets, real_batch
        assert calls == ([("sets", [None, 9, None, None, 9, 9])] if shared else [])
        for i in (1, 5, 6):
            assert tickets[i]._view.set_id == 9 and tickets[i]._view.n == SET_ROWS.size and tickets[i]._avg.shape == (SET_ROWS.size, 2)
        assert (tickets[3]._n_e[:, 0] == 2).all() and (tickets[3]._n_e[:, 1] == 3).all()
        out.append((db, tickets))
    (db_b, tk_b), (db_s, tk_s) = out
    band = tk_s[0]._review_band(hp)
    for i, (b, s) in enumerate(zip(tk_b, tk_s)):
        solo = np.asarray(s._ahead["scores"])
        assert np.abs(solo - band[0]).min() > 1e-9 and np.abs(solo - band[1]).min() > 1e-9, i          # the fixture keeps scores off the band
        assert np.asarray(b._avg).shape == np.asarray(s._avg).shape and np.abs(np.asarray(b._avg) - np.asarray(s._avg)).max() <= TOL, i
        assert np.abs(np.asarray(b._ahead["scores"]) - solo).max() <= TOL, i
        assert (np.asarray(b._n_e) == np.asarray(s._n_e)).all(), i
        assert (b._ahead["match_rows"] == s._ahead["match_rows"]).all() and (b._ahead["near_rows"] == s._ahead["near_rows"]).all(), i
        assert b._ahead["near_argmax"] == s._ahead["near_argmax"] and b._ahead["select"] == s._ahead["select"], i
        assert list(b.similarities) == list(s.similarities)
    assert len(tk_b[1]._ahead["match_rows"]) + len(tk_b[1]._ahead["near_rows"]) > 0
    # other weights after the shared pass: the ticket's own similarities go back to the device under its own set first
    tk = tk_b[5]
    tk.compute_scores({"rgb": 1.0, "warped_optical_flow": 0.7})
    assert db_b.search_set_in_use == 9 and db_b.sims_owner is tk._round
    db_s.use_search_set(9)
    db_s.restrict_slots(None)
    db_s.write_avg(np.asarray(tk._avg), np.asarray(tk._n_e))
    want = db_s.query_round(None, weights=np.array([1.0, 0.7]), select=band)
    assert (np.asarray(tk._score_values) == np.asarray(want.scores)).all() and want.scores.shape == (SET_ROWS.size,)
    assert (tk._ahead["match_rows"] == want.match_rows).all() and (tk._ahead["near_rows"] == want.near_rows).all()
    assert tk._ahead["near_argmax"] == want.near_argmax and tk._ahead["select"] == band
    db_b.close()
    db_s.close()


def _run(vqa, db, pairs, **kw):
    """compute_matches over ``pairs`` -> (tickets, hp, the (threshold, lower, scores) of every selection, query_round_batch_sets calls)."""
    made, bands, calls = [], [], []
    real_init, real_select, real_sets = vqa.Ticket.__init__, vqa.Ticket.select_clips_to_review, type(db).query_round_batch_sets

    def init(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)

    def select(self, threshold=0.8, max_number_matches=20, near_miss=0.5):
        bands.append((threshold, threshold - near_miss * (1 - threshold), np.array(self._score_values)))
        return real_select(self, threshold, max_number_matches, near_miss)

    def spy_sets(self, targets, *a, **k):
        calls.append(len(targets))
        return real_sets(self, targets, *a, **k)
    vqa.Ticket.__init__, vqa.Ticket.select_clips_to_review, type(db).query_round_batch_sets = init, select, spy_sets
    hp = make_hp(vqa)
    try:
        random.seed(a=SEED)
        vqa.compute_matches(Repo(pairs), hp, **kw)
    finally:
        vqa.Ticket.__init__, vqa.Ticket.select_clips_to_review, type(db).query_round_batch_sets = real_init, real_select, real_sets
    return made, hp, bands, calls


def test_compute_matches_sharing_search_sets_equals_the_default_path(vqa):
    """Two new updates on search set 9, one on the whole database, a revise and a finalize: compute_matches(batch=True,
    share_search_sets=True) runs ONE pass for the five and posts the review sets of the default path (compare_runs of
    tests/test_batch_tickets_gpu.py: same clips in the same order, values and hyperparameters within 1e-12, same ledgers)."""
    def pairs(db):
        later = {"latest_query_result": {"round": 1, "bootstrapped_target": None, "id": 3}}
        m3, u3 = labelled(REFS[3])
        m4, u4 = labelled(REFS[4])
        return [("new", update(db, REFS[0])), ("new", update(db, 502, search_set=9)), ("new", update(db, 904, search_set=9)),
                ("revise", update(db, REFS[3], matches=m3, user_matches=u3, **later)),
                ("finalize", update(db, REFS[4], matches=m4, user_matches=u4, **later))]
    db_s, db_b = resident(vqa), resident(vqa)
    for db in (db_s, db_b):
        db.define_search_rows(9, SET_ROWS)
    seq = _run(vqa, db_s, pairs(db_s))
    bat = _run(vqa, db_b, pairs(db_b), batch=True, share_search_sets=True)
    assert seq[3] == [] and bat[3] == [5]
    assert [len(tk.scores) for tk in bat[0]] == [base.N, SET_ROWS.size, SET_ROWS.size, base.N, base.N]
    compare_runs(seq, bat)
    db_s.close()
    db_b.close()
