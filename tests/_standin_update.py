"""Test infrastructure: the numpy stand-in database of tests/test_batch_fit_standin.py plus FeatureDB.batch_round_update restated on the
host -- raw_loss_surface + Hyperparameter._pick_exact + the band expressions of compute_matches._review_budget and
select_clips_to_review.  Never imported by the product."""
import numpy as np

import sim_oracle as so
from _pick_cases import compute_eps, make_hp
from _search_set_cases import np_select
from test_batch_fit_standin import LATER, FitOracleFeatureDB
from test_batch_tickets_standin import IDS, _hp, _ticket, _update

import video_query_algorithms_amd as vqa
from video_query_algorithms_amd.feature_db import UpdateResult
from video_query_algorithms_amd.hyperparameter import raw_loss_surface


def host_band(th, reach, lowest_of, eps):
    """(lowest, (threshold, lower)): ``reach`` None = a finalize member, whose reach comes from ``lowest_of()``."""
    lowest = 1.0
    if reach is None:
        lowest = lowest_of()
        reach = max(th - lowest, 0) / max(1 - th, eps)
    return lowest, (float(th), float(th - reach * (1 - th)))


class UpdateOracleFeatureDB(FitOracleFeatureDB):
    """``picks`` keeps (query, surface / L, the _pick_exact result) of every member served, for the tests to compare with _pick_from."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.picks = []

    def batch_round_update(self, queries, rows, labels, w_grids, th_grids, ballasts, seconds, eps, reaches, user_rows, want_scores=True,
                           want_surface=False, surfaces=None):
        self.log.append(("update", list(queries)))
        assert eps == compute_eps()
        hp = make_hp(vqa)
        out = []
        for i, q in enumerate(queries):
            avg = self._kept[q][0]
            wg = np.asarray(w_grids[i])
            assert np.array_equal(wg[:, seconds[i]], hp.weight_grid) and np.array_equal(th_grids[i], hp.threshold_grid)
            graded = np.stack([so.dense_scores(avg[np.asarray(rows[i], dtype=np.int64)], w) for w in wg])
            surface = raw_loss_surface(graded, labels[i], th_grids[i], ballasts[i]) / len(labels[i])
            picked = hp._pick_exact(surface)
            self.picks.append((q, surface, picked))
            r = UpdateResult()
            r.avg, r.n_e = self._kept[q]
            r.w, r.threshold, r.iw, r.it, r.on_rim, r.fell_back = (picked[0][hp.streams[1]],) + picked[1:]
            w = np.array(wg[r.iw])
            w[seconds[i]] = r.w
            r.scores = so.dense_scores(avg, w)
            assert list(user_rows[i]) == sorted(user_rows[i]) and (reaches[i] is None or not len(user_rows[i]))

            def lowest_of(scores=r.scores, at=user_rows[i]):
                m = 1
                for row in at:
                    m = min(m, scores[row])
                return m
            r.lowest, r.band = host_band(r.threshold, reaches[i], lowest_of, eps)
            r.match_rows, r.near_rows, r.near_argmax = np_select(r.scores, *r.band)
            r.surface = None
            out.append(r)
        return out


def labelled_inside(db, row, kind="revise", w=1.3, count=24):
    """A revise / finalize update on clip ``row`` whose verdicts put the minimum of the loss surface INSIDE the grid for most rows
    (the verdicts of test_batch_tickets_standin._labelled leave it in the corner): the ``count`` best clips under weight ``w``, the
    better half confirmed, one verdict in eight flipped."""
    hp = _hp()
    hp.weights, hp.threshold = {"rgb": 1.0, "warped_optical_flow": w}, 0.8
    tk = _ticket(db, row, hp)
    tk.compute_similarities(hp)
    tk.compute_scores(hp.weights)
    v = np.array(tk._score_values)
    order = np.argsort(-v)[:count]
    cut = v[order[count // 2]]
    rng = np.random.default_rng(row)
    matches, user = [], {}
    for r in order:
        verdict = bool(v[r] >= cut) ^ bool(rng.random() < 0.12)
        matches.append({"video_clip": int(IDS[r]), "user_match": verdict, "is_match": bool(v[r] >= 0.8)})
        user[str(int(IDS[r]))] = verdict
    user[str(int(IDS[row]))] = True
    return (kind, _update(row, feature_db=db, matches=matches, user_matches=user, **LATER))
