"""GPU: compute_matches(batch=True, fit_weights=True) on a resident FeatureDB -- the weight update of a group's revise and finalize
tickets in one batch_round_fit and one batch_round_rescore behind the group's pass -- against compute_matches(batch=True) on a second,
identical database (value for value: both fit on the pass's similarities) and against the unbatched compute_matches (to rounding)."""
import random

import numpy as np
import pytest

import sim_oracle as so
import test_batch_tickets_gpu as base
from _helpers import SEED
from _search_set_cases import host_loss_surface

pytestmark = pytest.mark.gpu
LATER = {"latest_query_result": {"round": 1, "bootstrapped_target": None, "id": 3}}
# revise tickets: (reference clip, where the oracle's loss surface has its minimum under the labels of base.labelled)
REVISE = ((base.REFS[3], "rim"), (base.REFS[0], "interior"), (37, "interior"))
FINALIZE = base.REFS[4]
COUNTED = ("query_round_batch", "query_round_batch_sets", "batch_round_fit", "batch_round_rescore", "write_avg", "loss_surface", "scores_grid",
           "query_round", "rescore", "select")


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    if base.X is None:
        base.X = base.features()
    return m


def updates(db, sets=None):
    """The mix of tests/test_batch_tickets_gpu.py -- three new updates, a revise, a finalize -- with two more revise updates.  ``sets``:
    the search set of each of the seven (None: the whole database)."""
    sets = sets or [None] * 7
    pairs = [("new", base.update(db, r)) for r in base.REFS[:3]]
    for row, _where in REVISE:
        m, u = base.labelled(row)
        pairs.append(("revise", base.update(db, row, matches=m, user_matches=u, **LATER)))
    m, u = base.labelled(FINALIZE)
    pairs.insert(4, ("finalize", base.update(db, FINALIZE, matches=m, user_matches=u, **LATER)))
    for (_kind, upd), sid in zip(pairs, sets):
        if sid is not None:
            upd["search_set"] = sid
    return pairs


def run(vqa, db, pairs, **kw):
    """compute_matches over ``pairs`` -> (tickets, hp, the (threshold, lower, scores) of every selection, the counted FeatureDB calls):
    the tuple base.compare_runs reads."""
    made, bands, calls = [], [], []
    cls = type(db)
    real_init, real_select = vqa.Ticket.__init__, vqa.Ticket.select_clips_to_review
    real = {name: getattr(cls, name) for name in COUNTED}

    def init(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)

    def select(self, threshold=0.8, max_number_matches=20, near_miss=0.5):
        bands.append((threshold, threshold - near_miss * (1 - threshold), np.array(self._score_values)))
        return real_select(self, threshold, max_number_matches, near_miss)

    def counted(name):
        def call(self, *a, **k):
            calls.append(name)
            return real[name](self, *a, **k)
        return call
    vqa.Ticket.__init__, vqa.Ticket.select_clips_to_review = init, select
    for name in COUNTED:
        setattr(cls, name, counted(name))
    hp = base.make_hp(vqa)
    try:
        random.seed(a=SEED)
        vqa.compute_matches(base.Repo(pairs), hp, **kw)
    finally:
        vqa.Ticket.__init__, vqa.Ticket.select_clips_to_review = real_init, real_select
        for name in COUNTED:
            setattr(cls, name, real[name])
    return made, hp, bands, calls


def outcome(made, hp):
    return ([tk.ledger for tk in made], [list(tk.matches.items()) for tk in made], dict(hp.weights), hp.threshold)


def oracle_minimum(hp, row):
    """(iw, it, on the rim, refined) of the loss surface the CPU oracle gives the labels of base.labelled(row)."""
    matches, _user = base.labelled(row)
    t = np.stack([[so.scale_feature(base.X[row, s, e].astype(np.float64)) for e in range(3)] for s in range(2)])
    _, avg, _ = so.dense_similarities(base.X, t)
    ids = base.IDS.tolist()
    rows = [ids.index(m["video_clip"]) for m in matches]
    y = [m["is_match"] if m["user_match"] is None else m["user_match"] for m in matches]
    cand = np.zeros((len(hp.weight_grid), 2))
    cand[:, 0], cand[:, 1] = 1.0, hp.weight_grid
    graded = np.stack([so.dense_scores(avg[rows], w) for w in cand])
    surface = host_loss_surface(graded, y, hp.threshold_grid, hp.ballast) / len(y)
    iw, it = np.unravel_index(np.argmin(surface), surface.shape)
    rim = iw in (0, len(hp.weight_grid) - 1) or it in (0, len(hp.threshold_grid) - 1)
    refined = (not rim) and tuple(hp._refine(surface, iw, it)) != (hp.weight_grid[iw], hp.threshold_grid[it])
    return int(iw), int(it), rim, refined


def test_the_labels_reach_both_branches_of_the_pick(vqa):
    """From the oracle's own surface: the minimum of the first revise ticket lies on the rim of the grid (taken as it is), those of
    the other two inside it, where _refine moves them off the grid."""
    hp = base.make_hp(vqa)
    for row, where in REVISE:
        iw, it, rim, refined = oracle_minimum(hp, row)
        assert (rim, refined) == ((True, False) if where == "rim" else (False, True)), (row, iw, it)


def check_fitted_run(vqa, fit, bat):
    made_f, hp_f, _bands, _calls = fit
    made_b, hp_b, _bands_b, _calls_b = bat
    assert [tk.ledger["process_state"] for tk in made_f] == [[3, 4]] * 4 + [[3, 7]] + [[3, 4]] * 2
    assert outcome(made_f, hp_f) == outcome(made_b, hp_b) and all(len(tk.matches) > 0 for tk in made_f)
    by_row = {tk.query_id: tk for tk in made_f}
    eps = float(__import__("os").environ["COMPUTE_EPS"])
    for row, where in REVISE:
        weights, th = by_row[row]._fit
        w = weights["warped_optical_flow"]
        on_grid = bool(np.isin(w, hp_f.weight_grid)) and np.abs(hp_f.threshold_grid - (th + eps)).min() < 1e-12
        if where == "rim":
            assert on_grid and (w in (hp_f.weight_grid[0], hp_f.weight_grid[-1]) or not hp_f.threshold_grid[0] + 1e-9 < th + eps < hp_f.threshold_grid[-1] - 1e-9)
        else:
            assert not on_grid and hp_f.weight_grid[0] < w < hp_f.weight_grid[-1]
    assert by_row[FINALIZE]._fit is not None and all(by_row[r]._fit is None for r in base.REFS[1:3])


def test_fitted_group_equals_the_batched_run_and_the_unbatched_one(vqa):
    """Seven updates in one pass: ledgers, matches (clip -> score), weights and threshold == those of compute_matches(batch=True), and
    within 1e-12 of the unbatched compute_matches under base.compare_runs' condition.  The fitted group asks the database for one
    pass, one fit, one rescore and the finalize ticket's own partition -- no write_avg, loss_surface or one-query round for a revise
    ticket."""
    dbs = [base.resident(vqa) for _ in range(3)]
    fit = run(vqa, dbs[0], updates(dbs[0]), batch=True, fit_weights=True)
    bat = run(vqa, dbs[1], updates(dbs[1]), batch=True)
    seq = run(vqa, dbs[2], updates(dbs[2]))
    check_fitted_run(vqa, fit, bat)
    assert fit[3] == ["query_round_batch", "batch_round_fit", "batch_round_rescore", "write_avg", "rescore", "select"]
    assert bat[3].count("loss_surface") == 4 and bat[3].count("write_avg") == 4 and bat[3].count("query_round") == 8
    base.compare_runs(seq, fit)
    for db in dbs:
        db.close()


def test_fitted_group_over_shared_search_sets(vqa):
    """The same with a search set per ticket and share_search_sets=True: one pass over the union, the fit and the rescore with rows
    as positions in each ticket's view."""
    needed = set()
    for row in [r for r, _ in REVISE] + [FINALIZE] + list(base.REFS):
        needed.add(row)
        needed.update(base.IDS.tolist().index(m["video_clip"]) for m in base.labelled(row)[0])
    sets = {"A": np.array(sorted(set(range(0, base.N, 2)) | needed)), "B": np.array(sorted(set(range(1, base.N, 2)) | needed))}
    assign = ["A", "B", None, "A", "B", "A", "B"]
    out = []
    for kw in ({"fit_weights": True}, {}):
        db = base.resident(vqa)
        for sid, rows in sets.items():
            db.define_search_rows(sid, rows)
        out.append(run(vqa, db, updates(db, assign), batch=True, share_search_sets=True, **kw))
        db.close()
    fit, bat = out
    made_f, hp_f = fit[0], fit[1]
    assert outcome(made_f, hp_f) == outcome(bat[0], bat[1]) and all(len(tk.matches) > 0 for tk in made_f)
    assert [tk._view.set_id for tk in made_f] == assign and all(tk._fit is not None for tk in made_f if tk.query_id in (37, FINALIZE))
    assert fit[3] == ["query_round_batch_sets", "batch_round_fit", "batch_round_rescore", "write_avg", "rescore", "select"]
    assert bat[3][0] == "query_round_batch_sets" and bat[3].count("loss_surface") == 4
