"""CPU: ticket.compute_similarities_batch(..., share_search_sets=True) on the numpy stand-in database -- which groups share a pass over
the union of their search sets (the rule sum M_q >= 2 * distinct), in which order things run, and that every ticket comes out as from
its own round (what the device adds is covered by tests/test_batch_tickets_sets_gpu.py)."""
import random

import numpy as np

import sim_oracle as so
from _helpers import DEFAULT_WEIGHTS, SEED
from test_batch_tickets_standin import IDS, N, X, RoundOracleFeatureDB, _db, _hp, _ticket, _who

import video_query_algorithms_amd as vqa
from video_query_algorithms_amd import ticket as ticket_mod
from video_query_algorithms_amd.feature_db import RoundResult

TOL = 1e-12


class SetsOracleFeatureDB(RoundOracleFeatureDB):
    """RoundOracleFeatureDB plus FeatureDB.query_round_batch_sets / search_set_view, restated from the oracle: every query over the rows
    of its own set, results indexed by position in it.  The set in use is neither consulted nor changed."""

    def search_set_view(self, set_id):
        if set_id is None:
            in_use, calls = self._in_use, self.use_calls
            view = self.use_search_set(None) if self._whole is None else self._whole
            if self._whole is not None and in_use is not None:
                self._in_use, self.use_calls = in_use, calls
            return view
        return self._sets[set_id]

    def query_round_batch_sets(self, targets, weights, set_ids, selects=None, want_avg=True, timed=False):
        if not 1 <= len(targets) <= 16:
            raise ValueError("1 to 16 queries per pass")
        self.log.append(("sets", [np.array(t) for t in targets], list(set_ids)))
        base = super(RoundOracleFeatureDB, self)._effective() if self._in_use is None else None
        if base is None:
            in_use = self._in_use
            self._in_use = None
            base = self._effective()
            self._in_use = in_use
        out = []
        for q, (t, w, sid) in enumerate(zip(targets, weights, set_ids)):
            rows = np.arange(self.n) if sid is None else self._sets[sid].rows
            _, avg, ne = so.dense_similarities(self.x[rows], t, None if base is None else base[rows])
            r = RoundResult()
            r.avg, r.n_e, r.scores = (avg if want_avg else None), ne, so.dense_scores(avg, w)
            self._select(r, None if selects is None else (float(selects[q][0]), float(selects[q][1])))
            out.append(r)
        return out


def _sdb():
    return _db(SetsOracleFeatureDB)


def _spy(tickets):
    order = []
    for i, tk in enumerate(tickets):
        own = tk.compute_similarities

        def spy(hyperparameters, _own=own, _i=i):
            order.append(_i)
            return _own(hyperparameters)
        tk.compute_similarities = spy
    return order


def _passes(db, tickets, kind):
    return [[_who(tickets, t) for t in entry[1]] for entry in db.log if entry[0] == kind]


def test_with_the_keyword_off_search_set_tickets_run_alone_as_ever():
    hp = _hp()
    a = _sdb()
    a.define_search_rows(77, np.arange(10, 200))
    tickets = [_ticket(a, r, hp) for r in range(0, 3)] + [_ticket(a, r, hp, search_set=77) for r in (20, 21, 22)]
    order = _spy(tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp)
    assert order == [3, 4, 5] and _passes(a, tickets, "batch") == [[0, 1, 2]] and _passes(a, tickets, "sets") == []
    assert [e[0] for e in a.log].count("scan") == 3


def test_the_sharing_rule_group_by_group():
    hp = _hp()
    # three tickets on one set, 3 M >= 2 M: one pass
    a = _sdb()
    a.define_search_rows(77, np.arange(10, 200))
    tickets = [_ticket(a, r, hp, search_set=77) for r in (20, 21, 22)]
    order = _spy(tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
    assert order == [] and _passes(a, tickets, "sets") == [[0, 1, 2]] and a.log[-1][2] == [77, 77, 77]
    assert a._in_use is None and a.sims_owner is None and a.scores_owner is None
    assert all(tk._view.set_id == 77 and tk._view.n == 190 and len(tk.similarities) == 190 and tk._ahead is not None for tk in tickets)
    # two tickets on two disjoint sets, sum = distinct: each alone, in list order
    b = _sdb()
    b.define_search_rows("x", np.arange(0, 100))
    b.define_search_rows("y", np.arange(100, 250))
    tickets = [_ticket(b, 5, hp, search_set="x"), _ticket(b, 120, hp, search_set="y")]
    order = _spy(tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
    assert order == [0, 1] and _passes(b, tickets, "sets") == [] and [e[0] for e in b.log] == ["scan", "scan"]
    # one whole-database ticket plus one half-size set, 1.5 N < 2 N: not shared
    c = _sdb()
    c.define_search_rows("half", np.arange(0, N, 2))
    tickets = [_ticket(c, 5, hp), _ticket(c, 120, hp, search_set="half")]
    order = _spy(tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
    assert order == [1, 0] and _passes(c, tickets, "sets") == [] and _passes(c, tickets, "batch") == []
    # two whole-database tickets plus three 10 % sets: 2 N + 0.3 N >= 2 N: one pass of five
    d = _sdb()
    for k in range(3):
        d.define_search_rows("tenth%d" % k, np.arange(k * 100, k * 100 + N // 10))
    tickets = [_ticket(d, 5, hp), _ticket(d, 20, hp, search_set="tenth0"), _ticket(d, 6, hp), _ticket(d, 130, hp, search_set="tenth1"),
               _ticket(d, 230, hp, search_set="tenth2")]
    order = _spy(tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
    assert order == [] and _passes(d, tickets, "sets") == [[0, 1, 2, 3, 4]] and d.log[-1][2] == [None, "tenth0", None, "tenth1", "tenth2"]
    assert [tk._view.n for tk in tickets] == [N, 30, N, 30, 30]
    # seventeen tickets on one set: a pass of 16, then the last alone
    e = _sdb()
    e.define_search_rows(1, np.arange(50, 250))
    tickets = [_ticket(e, r, hp, search_set=1) for r in range(60, 77)]
    order = _spy(tickets)
    vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
    assert order == [16] and _passes(e, tickets, "sets") == [list(range(16))]
    # another slot mask: its own group
    f = _sdb()
    f.define_search_rows(1, np.arange(50, 250))
    tickets = [_ticket(f, r, hp, search_set=1) for r in (60, 61)] + [_ticket(f, r, hp, search_set=1, drop=("warped_optical_flow", 2)) for r in (62, 63)]
    order = _spy(tickets)
    calls = f.restrict_calls
    vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
    assert order == [] and _passes(f, tickets, "sets") == [[0, 1], [2, 3]] and f.restrict_calls == calls + 2
    assert tickets[2].similarities[int(IDS[50])]["warped_optical_flow"][1] == 2


def _round_of(tk, hp, weights):
    tk.compute_scores(weights)
    tk.select_clips_to_review(hp.threshold, tk.number_of_matches_to_review, hp.near_miss_default)
    return list(tk.matches.items())


def test_shared_and_one_by_one_rounds_agree_and_consume_random_identically():
    hp = _hp()
    hp.weights, hp.threshold = dict(DEFAULT_WEIGHTS), 0.8
    other = {"rgb": 1.0, "warped_optical_flow": 0.75}
    out, states = [], []
    for shared in (True, False):
        db = _sdb()
        db.define_search_rows("s", np.arange(3, 260))
        db.define_search_rows("t", np.arange(40, 300, 2))
        tickets = [_ticket(db, 17, hp, search_set="s"), _ticket(db, 42, hp, search_set="t"), _ticket(db, 99, hp, search_set="s"),
                   _ticket(db, 150, hp), _ticket(db, 200, hp, search_set="t"), _ticket(db, 210, hp)]
        if shared:
            vqa.ticket.compute_similarities_batch(tickets, hp, share_search_sets=True)
            assert [e[0] for e in db.log] == ["sets"] and len(db.log[0][1]) == 6
        else:
            for tk in tickets:
                tk.compute_similarities(hp)
        random.seed(a=SEED)
        got = []
        for tk in tickets:
            scans = len(db.log)
            first = _round_of(tk, hp, DEFAULT_WEIGHTS)
            assert len(db.log) == scans                       # looked-ahead arguments: nothing asked of the database
            got.append((tk._view.set_id, tk._view.n, np.array(tk._avg), np.array(tk._n_e), np.array(tk._score_values), first,
                        _round_of(tk, hp, other)))            # other weights: the ticket's own similarities go back under its own set
        out.append(got)
        states.append(random.getstate())
    assert states[0] == states[1]                             # `random` consumed identically
    for (sid_b, n_b, avg_b, ne_b, sc_b, m_b, m2_b), (sid_s, n_s, avg_s, ne_s, sc_s, m_s, m2_s) in zip(*out):
        assert sid_b == sid_s and n_b == n_s and avg_b.shape == avg_s.shape == (n_b, 2)
        assert np.abs(avg_b - avg_s).max() <= TOL and (ne_b == ne_s).all() and np.abs(sc_b - sc_s).max() <= TOL
        assert [c for c, _ in m_b] == [c for c, _ in m_s] and [c for c, _ in m2_b] == [c for c, _ in m2_s] and len(m_b) > 0
        assert max(abs(v - w) for (_, v), (_, w) in zip(m_b + m2_b, m_s + m2_s)) <= TOL
    assert ticket_mod.SHARE_SETS_FACTOR == 2 and ticket_mod.BATCH_PASS == 16
