"""Drop-in for the reference's ``compute_matches`` (src/models/compute_matches.py:8-107).

The orchestration of one broker pass: every pending query update becomes a ticket, gets its target, is scanned,
re-weighted, scored and turned into the next review set.  The sequence of calls on the ticket is the reference's (so
the REST side effects of its Ticket methods happen in the same order); the arithmetic behind ``compute_similarities``,
``optimize_weights``, ``compute_scores`` and ``select_clips_to_review`` runs on the GPU (``TicketScoring``,
``Hyperparameter``, ``TargetClip``).  ``ticket_factory(update_object, url)`` supplies the Ticket class -- the reference's
own, patched by ``install``, or the offline ``Ticket``.

In production this module is NOT needed: after ``install()`` the reference's own ``compute_matches.py`` runs
unmodified on the patched classes.  It exists as the offline harness -- a broker pass with no REST
server (tests, ``tools/e2e_cfg5.py``): with no ``ticket_factory`` every update object carries its own search set
(``records`` and/or ``feature_db``) and the side effects land in ``Ticket.ledger``.
"""
from __future__ import annotations

import os

from .target_clip import TargetClip, solve_targets_batch

_IN_PROGRESS, _PROCESSED, _ERROR, _FINALIZED = 3, 4, 5, 7      # process states, compute_matches.py:42,50,104,107


def _choose_weights(kind, update, tk, hp):
    """compute_matches.py:60-67: defaults for a new query (or one without matches yet), else re-fit on the labels."""
    if kind == "new" or not update["matches"]:
        hp.weights = hp.default_weights
        hp.threshold = hp.default_threshold
    elif kind in ("revise", "finalize"):
        fit = getattr(tk, "_fit", None)
        if fit is not None and getattr(tk, "_fit_round", None) is tk._round:
            hp.weights, hp.threshold = fit                                  # fitted behind this round's batched pass (fit_weights)
        else:
            hp.optimize_weights(tk)
    else:
        raise Exception('update type is invalid')


def _review_budget(kind, tk, hp):
    """compute_matches.py:78-88: (how many matches go out, how far below the threshold to look).  A finalize pass
    reports everything and reaches down to the lowest-scoring match the user confirmed."""
    if kind != "finalize":
        return tk.number_of_matches_to_review, hp.near_miss_default
    lowest, _clip = tk.lowest_scoring_user_match()
    reach = max(hp.threshold - lowest, 0) / max(1 - hp.threshold, float(os.environ["COMPUTE_EPS"]))
    return float("inf"), reach


def _begin_update(kind, update, url, hp, ticket_factory, target_factory, plan_only=False):
    """Phase 1 of a round: the ticket, process state 3, the consistency checks (:47-52) and the target's features (:55-56).  Returns
    the ticket, or None when the round ended with a fatal error.  ``plan_only``: a target that can plan its round
    (``plan_target_features``: the REST requests and the draws) does just that; the caller solves the planned targets together."""
    tk = ticket_factory(update, url)
    tk.change_process_state(_IN_PROGRESS)
    fatal, warning = tk.catch_errors(kind)                                  # :47-52
    if fatal:
        tk.change_process_state(_ERROR, message=fatal)
        return None
    if warning:
        tk.add_note(warning)

    tk.target = target_factory(tk, hp)                                      # :55-58
    if plan_only and hasattr(tk.target, "plan_target_features"):
        tk.target.plan_target_features()
    else:
        tk.target.get_target_features()
    return tk


def _finish_update(kind, update, tk, hp):
    """The round behind compute_similarities: weights, the query result, scores, the review set and its side effects (:60-107)."""
    _choose_weights(kind, update, tk, hp)

    round_no = 1 if kind == 'new' else tk.latest_query_result["round"] + 1  # :70-74
    result_id = tk.create_query_result(round_no, hp)

    tk.compute_scores(hp.weights)                                           # :77
    budget, reach = _review_budget(kind, tk, hp)
    tk.select_clips_to_review(hp.threshold, budget, reach)
    if not tk.matches:                                                      # :92-94
        catch_no_matches_error(tk)
        return
    tk.add_matches_to_database(result_id)                                   # :97
    if kind == "finalize":                                                  # :102-107
        tk.create_final_report(hp, result_id)
        tk.change_process_state(_FINALIZED)
    else:
        tk.change_process_state(_PROCESSED)


def _one_update(kind, update, url, hp, ticket_factory, target_factory):
    tk = _begin_update(kind, update, url, hp, ticket_factory, target_factory)
    if tk is None:
        return
    tk.compute_similarities(hp)
    _finish_update(kind, update, tk, hp)


def compute_matches(query_updates, hyperparameters, ticket_factory=None, target_factory=TargetClip, batch=False, share_search_sets=False,
                    fit_weights=False, batch_targets=False, top=None):
    """One broker pass.  ``batch=True`` runs it in three phases so that the pending tickets share passes over their resident database
    (``ticket.compute_similarities_batch``): (1) every pending update gets its ticket, process state 3, its checks and its target
    features; (2) ONE ``compute_similarities_batch`` over the tickets that survived; (3) every ticket is finished in the original
    order.  Per ticket the calls -- and with them the ledger -- are the same sequence as without ``batch``; ACROSS tickets they
    interleave differently (all the phase-1 entries come before any ticket's phase-3 entries), and a ticket's weights / threshold
    look-ahead is taken from the hyperparameters object as it stands before phase 3 changes it (a ticket whose weights come out
    different re-weights its own similarities, as ever).  Values agree with the default path to rounding (<= 1e-12).
    ``share_search_sets=True`` (with ``batch``): tickets whose search sets are defined on their database share passes too
    (``compute_similarities_batch(..., share_search_sets=True)``).
    ``fit_weights=True`` (with ``batch``; ``ValueError`` without): the revise and finalize updates that have ``matches`` get their
    weight update behind their group's pass, on the similarities it left on the device (``compute_similarities_batch(..., fit=...)``:
    two calls per group instead of four per ticket), and ``_choose_weights`` takes ``hp.weights`` / ``hp.threshold`` from the ticket's
    ``_fit``.  A ticket without one for its current round -- alone in its group, without a resident database, on a sharded one that was
    opened without ``batch_rounds=True``, without labels -- calls ``hp.optimize_weights`` as ever.  Per ticket the order of phase 3, the ledger and the consumption of
    ``random`` are unchanged; weights, threshold and matches are those of ``batch=True`` bit for bit (both fit on the pass's
    similarities).  Two differences: between the fit and ``compute_scores`` ``ticket.scores`` is not left at the last grid weight
    (compute_matches.py:77 overwrites it on the next line), and a finalize ticket's scores come back with the group's while its
    review band -- which depends on ``lowest_scoring_user_match`` under the fitted scores -- is still partitioned by its own
    ``select``.
    ``fit_weights="device"`` (with ``batch``): the same, with the group's update in ONE call where the database has
    ``batch_round_update`` -- a ``FeatureDB``, or a ``ShardedFeatureDB`` opened with ``batch_rounds=True``, where it is one operation of
    the sharded database -- (``compute_similarities_batch(..., fit_on_device=True)``): the pick and its refinement run on the device, and
    so does a finalize ticket's review band, which removes the second difference above.  One difference instead: weights and threshold
    are ``Hyperparameter._pick_exact``'s rather than ``_pick_from``'s (products instead of ``** 2``: equal in most picks, a few ulp apart
    in the others -- tests/test_pick_exact.py has the measured size); ledger, ``random`` consumption and matches are those of
    ``fit_weights=True`` whenever the two picks agree.
    ``batch_targets=True`` (with ``batch``; ``ValueError`` without): phase 1 only PLANS every ticket's target (the REST requests and the
    draws from ``random``, at the same place and in the same order as ever), and one ``target_clip.solve_targets_batch`` in front of
    the pass solves them: the tickets with ``dynamic_target_adjustment`` whose validated clips are rows of one resident database get
    every draw of their bootstrapping in ONE ``FeatureDB.batch_targets`` call per 16 tickets instead of one call per draw.  Per
    ticket the ledger, the consumption of ``random``, ``target_features``, weights, threshold and matches are those of
    ``batch=True`` bit for bit.  One difference: a solve that raises (a singular system, a key the previous target lacks) does so
    after every ticket of the pass has been planned, not in the middle of phase 1.
    ``top`` (with ``batch``; ``ValueError`` without): an int, or one per started ticket -- every ticket also gets the ``top`` best
    clips of its search set, ranked on the device behind its group's pass and fit (``compute_similarities_batch(..., top=...)``);
    ``ticket.top_clips(k)`` serves them.  Nothing else of the pass changes."""
    if top is not None and not batch:
        raise ValueError("top needs batch=True: the ranking is taken behind a batched pass")
    if fit_weights and not batch:
        raise ValueError("fit_weights=True needs batch=True: the fit runs behind a batched pass")
    if batch_targets and not batch:
        raise ValueError("batch_targets=True needs batch=True: the targets are solved together in front of a batched pass")
    pending = query_updates.get_status()                                    # :34
    if ticket_factory is None:
        from .ticket import Ticket as _Ticket

        def ticket_factory(update_object, url):
            # offline: the update object itself carries the search set (API feature records and/or a resident
            # FeatureDB); the REST side effects of the round are kept in the ticket's ledger
            return _Ticket(update_object, records=update_object.get("records"), feature_db=update_object.get("feature_db"))
    if not batch:
        for kind, update in pending.items():                                # :37
            if update is not None:
                _one_update(kind, update, query_updates.url, hyperparameters, ticket_factory, target_factory)
        return
    from .ticket import compute_similarities_batch
    started = []
    for kind, update in pending.items():
        if update is not None:
            tk = _begin_update(kind, update, query_updates.url, hyperparameters, ticket_factory, target_factory, plan_only=batch_targets)
            if tk is not None:
                started.append((kind, update, tk))
    if batch_targets:
        solve_targets_batch([tk.target for _kind, _update, tk in started])
    fit = [fit_weights and kind in ("revise", "finalize") and bool(update["matches"]) for kind, update, _tk in started]
    compute_similarities_batch([tk for _kind, _update, tk in started], hyperparameters, share_search_sets=share_search_sets,
                               **({"fit": fit} if fit_weights else {}), **({"top": top} if top is not None else {}),
                               **({"fit_on_device": True, "finalize": [kind == "finalize" for kind, _update, _tk in started]}
                                  if fit_weights == "device" else {}))
    for kind, update, tk in started:
        _finish_update(kind, update, tk, hyperparameters)


def catch_no_matches_error(ticket):
    """compute_matches.py:110-114."""
    which = ticket.latest_query_result["round"] if ticket.latest_query_result else 1
    ticket.change_process_state(_ERROR, message="*** Error: No matches were found for round {} of query {}! ***".format(
        which, ticket.query_id))
