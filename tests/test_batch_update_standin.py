"""CPU: compute_matches(batch=True, fit_weights="device") and ticket.compute_similarities_batch(fit=..., fit_on_device=True) on the numpy
stand-in database (tests/_standin_update.py): which members the one call serves, what it leaves to ask, and that the run is the
fit_weights=True run -- ledger, consumption of ``random``, matches -- wherever Hyperparameter._pick_exact and _pick_from agree bit for
bit, which the rows chosen here do (asserted).  The device side is covered by tests/test_batch_update_gpu.py."""
import logging
import random

import numpy as np
import pytest

from _standin_update import UpdateOracleFeatureDB, host_band, labelled_inside
from test_pick_exact import BOUND
from test_batch_fit_standin import LATER, FitOracleFeatureDB, _kinds, _mixed, _outcome, _revise, _run
from test_batch_tickets_standin import IDS, _db, _hp, _labelled, _ticket, _update

import video_query_algorithms_amd as vqa

ASKED = ("batch", "fit", "rescore", "update", "scan", "write_avg", "select", "scores_grid", "round")


def _picks_agree(db):
    """Every member the stand-in served was picked the same by _pick_from and _pick_exact, bit for bit."""
    hp = _hp()
    assert db.picks
    for _q, surface, (weights, th, _iw, _it, _rim, _fell) in db.picks:
        w_from, th_from = hp._pick_from(surface)
        if not (w_from == weights and np.float64(th_from).tobytes() == np.float64(th).tobytes()):
            return False
    return True


def test_one_call_updates_the_group_and_equals_the_two_call_run():
    db_d, made_d, hp_d = _run(_mixed, UpdateOracleFeatureDB, batch=True, fit_weights="device")
    after_d = random.random()
    db_f, made_f, hp_f = _run(_mixed, UpdateOracleFeatureDB, batch=True, fit_weights=True)
    after_f = random.random()
    assert _picks_agree(db_d) and [q for q, _s, _p in db_d.picks] == [2, 3, 5, 6]
    assert _outcome(made_d, hp_d) == _outcome(made_f, hp_f) and after_d == after_f
    assert [tk.ledger["process_state"] for tk in made_d] == [[3, 4], [3, 4], [3, 4], [3, 5], [3, 7], [3, 4], [3, 4], [3, 4]]
    # one pass and one update for the three revise tickets and the finalize one; the finalize ticket asks for nothing more
    assert _kinds(db_d, *ASKED) == ["batch", "update"] and [qs for kind, qs in db_d.log if kind == "update"] == [[2, 3, 5, 6]]
    assert _kinds(db_f, *ASKED) == ["batch", "fit", "rescore", "write_avg", "select"]     # the switch off: today's calls
    assert not db_f.picks
    for tk in made_d:
        assert (tk._fit is not None) == (tk.query_id in (60, 90, 150))


def _inside(db):
    return [("new", _update(5, feature_db=db)), labelled_inside(db, 33), labelled_inside(db, 210, "finalize"), labelled_inside(db, 90),
            ("new", _update(130, feature_db=db)), labelled_inside(db, 150, "finalize")]


def test_refined_picks_equal_the_two_call_run_too():
    """Verdicts that put the minimum inside the grid for rows 33 and 210 (refined on both paths to the same bits) and on its rim for
    rows 90 and 150: ledger, ``random`` and matches are those of fit_weights=True, and neither finalize ticket selects on its own."""
    db_d, made_d, hp_d = _run(_inside, UpdateOracleFeatureDB, batch=True, fit_weights="device")
    after_d = random.random()
    db_f, made_f, hp_f = _run(_inside, UpdateOracleFeatureDB, batch=True, fit_weights=True)
    after_f = random.random()
    assert [(q, p[4], p[5]) for q, _s, p in db_d.picks] == [(1, False, False), (2, False, False), (3, True, False), (5, True, False)]
    assert _picks_agree(db_d)
    assert _outcome(made_d, hp_d) == _outcome(made_f, hp_f) and after_d == after_f and all(tk.matches for tk in made_d)
    assert _kinds(db_d, *ASKED) == ["batch", "update"]
    assert _kinds(db_f, *ASKED) == ["batch", "fit", "rescore", "write_avg", "select", "write_avg", "select"]      # the switch off: today's calls


def test_a_pick_that_differs_stays_within_the_measured_bound():
    """Row 60 under these verdicts: _pick_from and _pick_exact refine the same cell to weights a few ulp apart (libm's pow against a
    product); the device mode takes _pick_exact's, within the bound of tests/test_pick_exact.py."""
    pairs = lambda db: [labelled_inside(db, 60), ("new", _update(5, feature_db=db))]         # noqa: E731
    db_d, made_d, hp_d = _run(pairs, UpdateOracleFeatureDB, batch=True, fit_weights="device")
    db_f, made_f, hp_f = _run(pairs, UpdateOracleFeatureDB, batch=True, fit_weights=True)
    (w_d, th_d), (w_f, th_f) = made_d[0]._fit, made_f[0]._fit
    got, want = np.array([w_d["warped_optical_flow"], th_d]), np.array([w_f["warped_optical_flow"], th_f])
    rel = np.abs(got - want) / np.abs(want)
    print("relative difference of (weight, threshold):", rel)
    assert (rel <= BOUND).all() and db_d.picks[0][2][2:] == (14, 7, False, False)
    assert [tk.ledger["process_state"] for tk in made_d] == [tk.ledger["process_state"] for tk in made_f]


def test_a_finalize_member_gets_its_band_from_the_device():
    """select_clips_to_review of the finalize ticket finds the partition of its own band in _ahead: no select call, and the band is the
    host's expression over the returned scores."""
    hp = _hp()
    db = _db(UpdateOracleFeatureDB)
    matches, user = _labelled(db, 60)
    tickets = [_ticket(db, 60, hp, matches=matches, user_matches=user), _ticket(db, 90, hp, matches=matches, user_matches=user), _ticket(db, 5, hp)]
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, True, False], fit_on_device=True, finalize=[True, False, False])
    assert _kinds(db, *ASKED) == ["batch", "update"]
    eps = float(__import__("os").environ["COMPUTE_EPS"])
    for tk, finalize in zip(tickets[:2], (True, False)):
        weights, th = tk._fit
        assert tk._fit_round is tk._round
        tk.compute_scores(weights)
        lowest, band = host_band(th, None if finalize else hp.near_miss_default, lambda: tk.lowest_scoring_user_match()[0], eps)
        assert tk._ahead["select"] == band and (lowest < 1.0) == finalize
        reach = max(th - lowest, 0) / max(1 - th, eps) if finalize else hp.near_miss_default
        tk.select_clips_to_review(th, float("inf") if finalize else 20, reach)
        assert tk.matches
    assert _kinds(db, *ASKED) == ["batch", "update"]                                         # nothing was asked behind the one call
    assert tickets[0]._ahead["select"] != tickets[1]._ahead["select"] or tickets[0]._fit[1] != tickets[1]._fit[1]
    assert tickets[2]._fit is None


def test_members_without_labels_or_with_an_unknown_clip_are_left_out():
    hp = _hp()
    db = _db(UpdateOracleFeatureDB)
    matches, user = _labelled(db, 60)
    stranger = [dict(matches[0], video_clip=999_999)] + matches[1:]
    tickets = [_ticket(db, 60, hp, matches=matches, user_matches=user), _ticket(db, 90, hp, matches=[]),
               _ticket(db, 150, hp, matches=stranger, user_matches=user), _ticket(db, 5, hp)]
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, True, True, False], fit_on_device=True, finalize=[False] * 4)
    assert [(kind, qs) for kind, qs in db.log if kind in ("fit", "rescore", "update")] == [("update", [0])]
    assert tickets[0]._fit is not None and all(tk._fit is None for tk in tickets[1:])
    # nobody labelled: no call at all
    db.log.clear()
    vqa.ticket.compute_similarities_batch(tickets[1:], hp, fit=[True, True, True], fit_on_device=True, finalize=[False, True, False])
    assert _kinds(db, *ASKED) == ["batch"]
    with pytest.raises(ValueError):
        vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True] * 4, fit_on_device=True)                     # finalize is needed
    with pytest.raises(ValueError):
        vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True] * 4, fit_on_device=True, finalize=[True])


def test_a_database_without_the_method_keeps_the_two_call_path():
    db_d, made_d, hp_d = _run(_mixed, FitOracleFeatureDB, batch=True, fit_weights="device")
    db_f, made_f, hp_f = _run(_mixed, FitOracleFeatureDB, batch=True, fit_weights=True)
    assert _kinds(db_d, *ASKED) == _kinds(db_f, *ASKED) == ["batch", "fit", "rescore", "write_avg", "select"]
    assert _outcome(made_d, hp_d) == _outcome(made_f, hp_f)


def test_a_ticket_alone_in_its_group_fits_on_its_own():
    db, made, hp = _run(lambda d: [_revise(d, 60, "finalize")], UpdateOracleFeatureDB, batch=True, fit_weights="device")
    ref_db, ref_made, ref_hp = _run(lambda d: [_revise(d, 60, "finalize")], UpdateOracleFeatureDB, batch=True)
    assert _kinds(db, "batch", "update", "scan", "scores_grid") == ["scan", "scores_grid"] and made[0]._fit is None
    assert _outcome(made, hp) == _outcome(ref_made, ref_hp)


def test_seventeen_tickets_update_behind_their_own_passes():
    rows = list(range(10, 10 + 17 * 9, 9))

    def pairs(db):
        return [_revise(db, r, "finalize" if i % 4 == 1 else "revise") for i, r in enumerate(rows)] + [("new", _update(200, feature_db=db))]
    db_d, made_d, hp_d = _run(pairs, UpdateOracleFeatureDB, batch=True, fit_weights="device")
    db_f, made_f, hp_f = _run(pairs, UpdateOracleFeatureDB, batch=True, fit_weights=True)
    assert [(kind, len(x)) for kind, x in db_d.log if kind in ("batch", "fit", "rescore", "update")] == \
        [("batch", 16), ("update", 16), ("batch", 2), ("update", 1)]
    assert not _kinds(db_d, "write_avg", "scores_grid", "select", "round", "scan")
    assert _kinds(db_f, "select").count("select") == 4                                        # the finalize tickets' own selects, switch off
    assert _picks_agree(db_d) and _outcome(made_d, hp_d) == _outcome(made_f, hp_f)
    assert int(IDS[rows[16]]) in made_d[16].matches


def test_the_fallback_of_the_refinement_is_logged_like_the_reference(caplog):
    class FellBack(UpdateOracleFeatureDB):
        def batch_round_update(self, *a, **kw):
            out = super().batch_round_update(*a, **kw)
            out[0].fell_back = True
            return out
    hp = _hp()
    db = _db(FellBack)
    matches, user = _labelled(db, 60)
    tickets = [_ticket(db, 60, hp, matches=matches, user_matches=user), _ticket(db, 5, hp)]
    with caplog.at_level(logging.WARNING):
        vqa.ticket.compute_similarities_batch(tickets, hp, fit=[True, False], fit_on_device=True, finalize=[False, False])
    assert [r.getMessage() for r in caplog.records] == ["hyperparameter quadratic fine tuning failed - resort to selecting optimum on grid "
                                                        "without further interpolation"]


def test_fit_weights_device_needs_batch():
    from test_batch_tickets_standin import _Repo
    with pytest.raises(ValueError):
        vqa.compute_matches(_Repo([]), _hp(), fit_weights="device")
