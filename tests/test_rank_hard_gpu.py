"""GPU: the one-query ranking kernels of csrc/vq_rank.hip (select_small / select_count / select_scan / select_scatter, topk_small /
topk_hist / topk_pick and the compaction with limit1, gather_scores) on the hard score rows of tests/_rank_cases.py, at every size cut.

The rows are PLANTED: written over the handle's scores on the device (FeatureDB.device_tensor("scores")), read back, and every
expectation is np_select / np_topk / np_min_score (tests/_search_set_cases.py) of what came back.  Every comparison is exact:
``array_equal`` on rows, ``same_bits`` on values.  One database per size serves all of that size's families, bands and k values
(``dbs``); tests/test_rank_cases.py shows on the CPU that this table tells nine wrong rankers from the right one.

The last test is about the host side of the same path: FeatureDB.query_round is two library calls when a list outgrows its 1024-row
prefix, and nothing of another thread may come between them."""
import ctypes as C
import sys
import threading
import time

import numpy as np
import pytest

import _rank_cases as rc
from _search_set_cases import np_min_score, np_select, np_topk, same_bits

pytestmark = pytest.mark.gpu
BIG_N = rc.SMALL_N + 1            # the smallest database that takes the three-pass partition and the radix top-k
CASES = [(n, fam) for n in rc.SIZES for fam in rc.families_at(n)]
SMALL_CASES = [(n, fam) for n, fam in CASES if n <= rc.SMALL_N]


def _ids(cases):
    return ["%d-%s" % c for c in cases]


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


class _Databases:
    """FeatureDB(n, 2, 1, 4) with scores on the handle, one per size; the BIG_N one stays, of the others the latest"""

    def __init__(self, vqa):
        self.vqa, self.held = vqa, {}

    def get(self, n):
        if n not in self.held:
            for old in [k for k in self.held if BIG_N not in (k, n)]:
                self.held.pop(old).close()
            db = self.vqa.FeatureDB(n, 2, 1, 4)
            with_scores(db, n)
            self.held[n] = db
        return self.held[n]

    def close(self):
        while self.held:
            self.held.popitem()[1].close()


@pytest.fixture(scope="module")
def dbs(vqa):
    d = _Databases(vqa)
    yield d
    d.close()


def with_scores(db, m):
    db.write_avg(np.zeros((m, 2)), np.ones((m, 2), dtype=np.int32))
    db.rescore([1.0, 0.0])


def plant(db, row):
    """the row over the handle's scores; returns what the device then holds (bit for bit the row)"""
    import torch
    dev = db.device_tensor("scores")
    assert tuple(dev.shape) == (row.size,)
    dev.copy_(torch.from_numpy(np.ascontiguousarray(row)))
    torch.cuda.synchronize()
    back = db.scores()
    assert same_bits(back, row)
    return back


def select_in_two_calls(vqa, db, th, lower):
    """vq_db_select, then vq_db_select_fetch into buffers of exactly the counts"""
    nm, nn, am = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5)
    vqa._lib.call("vq_db_select", db._h, float(th), float(lower), C.byref(nm), C.byref(nn), C.byref(am))
    m, q = np.full(nm.value, -7, dtype=np.int64), np.full(nn.value, -7, dtype=np.int64)
    vqa._lib.call("vq_db_select_fetch", db._h, m.ctypes.data_as(C.c_void_p) if m.size else None, m.size,
                  q.ctypes.data_as(C.c_void_p) if q.size else None, q.size)
    return m, q, am.value


def same_partition(got, want):
    return (got[0].dtype == np.int64 and got[1].dtype == np.int64 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and int(got[2]) == int(want[2]))


def check_partition(vqa, db, back, row, entries=2):
    """every band of the row through FeatureDB.select (vq_db_select_rows) and through vq_db_select + vq_db_select_fetch; returns the results"""
    out = []
    for name, th, lower in rc.bands_of(back):
        want = np_select(back, th, lower)
        got = db.select(th, lower)
        assert same_partition(got, want), (row.family, row.variant, row.n, name, th, lower, "select", [len(g) for g in got[:2]], got[2], want[2])
        if entries == 2:
            got = select_in_two_calls(vqa, db, th, lower)
            assert same_partition(got, want), (row.family, row.variant, row.n, name, th, lower, "select + fetch", got[2], want[2])
        out.append(got)
    return out


def check_topk(db, back, row, ks, order=None):
    """db.topk(k) against np_topk of the scores read back: rows, value bits, length min(k, n_valid)"""
    order = np_topk(back, back.size) if order is None else order
    out = []
    for k in ks:
        rows, vals = db.topk(k)
        assert rows.dtype == np.int64 and vals.dtype == np.float64 and len(rows) == len(vals) == min(k, order[0].size), (row.family, row.variant, row.n, k, len(rows))
        assert np.array_equal(rows, order[0][:k]), (row.family, row.variant, row.n, k, rows[:8], order[0][:8])
        assert same_bits(np.array(vals), order[1][:k]), (row.family, row.variant, row.n, k)
        out.append((np.array(rows), np.array(vals)))
    return out


# ------------------------------------------------------------------------------------------------------------------- the partition
@pytest.mark.parametrize("n,family", CASES, ids=_ids(CASES))
def test_partition_through_each_entry(vqa, dbs, n, family):
    """Lists, counts and near arg-max == np_select for every row of the family under every band, through both entries.  From 524 289
    rows on the carry loop of select_scan_block runs (257 and 513 blocks): with every row matching (the all_match band on rows
    without a NaN), with every row near (inf_neginf), and with the near arg-max in block 256 and in the last block (near_max_ties)."""
    db = dbs.get(n)
    for row in rc.rows_of(n, (family,)):
        back = plant(db, row.scores)
        check_partition(vqa, db, back, row)
        if family in ("all_equal", "ramp_up", "ramp_down"):
            m, q, _arg = db.select(-np.inf, -np.inf)
            assert np.array_equal(m, np.arange(n)) and q.size == 0
        if family == "near_max_ties":
            assert db.select(rc.TH, rc.LOWER)[2] == rc.near_max_pairs(n)[row.variant][0]          # the FIRST of the tied pair


@pytest.mark.parametrize("n,family", SMALL_CASES, ids=_ids(SMALL_CASES))
def test_one_workgroup_forms_and_general_forms_agree(vqa, dbs, n, family):
    """The same numbers in a database of n <= 16 384 rows (select_small_kernel, topk_small_kernel) and in one of 16 385 rows whose other
    rows are NaN (the three passes, the radix launch sequence): identical lists, counts, arg-max and k best."""
    small, big = dbs.get(n), dbs.get(BIG_N)
    for row in rc.rows_of(n, (family,)):
        padded = np.full(BIG_N, np.nan)
        padded[:n] = row.scores
        back = plant(small, row.scores)
        got_small = check_partition(vqa, small, back, row, entries=1)
        best_small = check_topk(small, back, row, rc.ks_of(back))
        back_big = plant(big, padded)
        got_big = [big.select(th, lower) for _name, th, lower in rc.bands_of(back)]
        best_big = [big.topk(k) for k in rc.ks_of(back)]
        for (name, _th, _lower), a, b in zip(rc.bands_of(back), got_small, got_big):
            assert same_partition(b, a), (family, row.variant, n, name)
        for k, a, b in zip(rc.ks_of(back), best_small, best_big):
            assert np.array_equal(a[0], b[0]) and same_bits(a[1], np.array(b[1])), (family, row.variant, n, k)
        assert same_bits(back_big[:n], back)


# ------------------------------------------------------------------------------------------------------------------- the k best
@pytest.mark.parametrize("n,family", CASES, ids=_ids(CASES))
def test_topk_in_both_forms(vqa, dbs, n, family):
    db = dbs.get(n)
    for row in rc.rows_of(n, (family,)):
        back = plant(db, row.scores)
        order = np_topk(back, n)
        ks = rc.ks_of(back)
        if row.variant == "ladder":                                       # and a k that stops the walk of every pass in every ladder digit
            ks = sorted(set(ks) | set(rc.ladder_ks(back).values()))
        got = dict(zip(ks, check_topk(db, back, row, ks, order)))
        if rc.SMALL_K + 1 <= n <= rc.SMALL_N:                             # k = 1024: one workgroup; k = 1025: the radix sequence
            a, b = got[rc.SMALL_K], got[rc.SMALL_K + 1]
            assert np.array_equal(a[0], b[0][:rc.SMALL_K]) and same_bits(a[1], b[1][:rc.SMALL_K])
        if family == "all_nan":
            assert all(r.size == 0 and v.size == 0 for r, v in got.values())
        if (family, row.variant) == ("signs", "mixed") and n >= 1023:
            rows, vals = got[n]
            zeros = rows[vals == 0.0]
            assert zeros.size >= 200 and (np.diff(zeros) > 0).all()        # -0 and +0 tie: position order
            assert np.signbit(vals[vals == 0.0]).any() and not np.signbit(vals[vals == 0.0]).all()
            assert vals[-1] == -np.inf and (vals[:-int((vals == -np.inf).sum())] > -np.inf).all()


@pytest.mark.parametrize("n", [rc.SMALL_N - 1, BIG_N])
def test_every_k_to_300_on_the_digit_ladder(vqa, dbs, n):
    """ladder: the k-th key sits in another (pass, digit) group every few k; last_byte: every k is decided in the eighth pass."""
    db = dbs.get(n)
    for row in rc.rows_of(n, ("digit_ladder",)):
        back = plant(db, row.scores)
        check_topk(db, back, row, range(1, 301), np_topk(back, 300))


# ------------------------------------------------------------------------------------------------------------------- min_score
def check_min_score(db, back, lists):
    for rows in lists:
        got, want = db.min_score(rows), np_min_score(back, rows)
        assert same_bits(np.float64(got), np.float64(want)), (list(rows)[:6], got, want)


def min_score_lists(back):
    """row lists with duplicates, NaN rows, -inf, scores above 1, both zeros in both orders, and the empty list"""
    rng = np.random.default_rng(back.size)
    nan, above, ninf = np.flatnonzero(np.isnan(back)), np.flatnonzero(back > 1), np.flatnonzero(back == -np.inf)
    pz, nz = np.flatnonzero((back == 0) & ~np.signbit(back)), np.flatnonzero((back == 0) & np.signbit(back))
    lists = [[], [0], [back.size - 1] * 3, nan[:5], above[:7], np.concatenate([above[:3], nan[:2], above[:3]]), rng.integers(0, back.size, 200),
             np.concatenate([above[:4], ninf[:1], above[:4]]), np.flatnonzero((back > 0) & (back < 1))[:9]]
    if pz.size and nz.size:
        lists += [[pz[0], nz[0]], [nz[0], pz[0]], [nz[0], nz[0], pz[0], above[0]]]
    return [np.asarray(v, dtype=np.int64) for v in lists]


@pytest.mark.parametrize("n", [65, 1025, BIG_N])
def test_min_score_of_row_lists(vqa, dbs, n):
    db = dbs.get(n)
    for row in rc.rows_of(n, ("signs", "digit_ladder", "one_number")):
        back = plant(db, row.scores)
        check_min_score(db, back, min_score_lists(back))
    mixed = plant(db, rc.rows_of(n, ("signs",))[0].scores)
    assert np.isnan(mixed).any() and (mixed > 1).any() and (mixed == -np.inf).any() == (n >= 16)
    assert db.min_score(np.flatnonzero(np.isnan(mixed))) == 1.0 and db.min_score([]) == 1.0


# ------------------------------------------------------------------------------------------------------------------- a search set
@pytest.mark.parametrize("m", [rc.SMALL_N - 1, BIG_N])
def test_ranking_under_a_search_set(vqa, m):
    """M rows out of 40 001 in use: the scores are [M], and select, topk and min_score rank POSITIONS of the set -- in the one-workgroup
    forms at M = 16 383, in the general ones at 16 385.  Then the whole database again."""
    n = 40001
    db = vqa.FeatureDB(n, 2, 1, 4)
    members = np.sort(np.random.default_rng(m).choice(n, m, replace=False)).astype(np.int64)
    view = db.define_search_rows("set", members)
    assert db.use_search_set("set") is view and view.n == m
    with_scores(db, m)
    for row in rc.rows_of(m):
        back = plant(db, row.scores)
        assert back.shape == (m,)
        check_partition(vqa, db, back, row)
        check_topk(db, back, row, rc.ks_of(back))
        if row.family == "signs":
            check_min_score(db, back, min_score_lists(back))
    with pytest.raises(vqa.VqError):
        db.min_score([m])                                                  # a position outside the set
    db.use_search_set(None)
    with_scores(db, n)
    for row in rc.rows_of(n, ("signs", "near_max_ties")):
        back = plant(db, row.scores)
        assert back.shape == (n,)
        check_partition(vqa, db, back, row)
        check_topk(db, back, row, rc.ks_of(back))
    db.drop_search_set("set")
    db.close()


# ------------------------------------------------------------------------------------------------------------------- the one-call round
TOP = 1040                         # the best scores of round_avg are distinct: a band can cut a list at any length up to here


def round_avg(n):
    """[n, 2] averaged similarities whose scores under the weights (1, 0) are 1 - |1 - avg[:, 0]|: TOP distinct best scores (multiples
    of 2^-12, exact through the square and the root), a two-valued body (near 0.2 and 0.3: long tie runs), NaN, -inf (from an infinite
    similarity and from a square that overflows) and large negatives down to -1e150"""
    rng = np.random.default_rng([7, n])
    a0 = np.where(rng.random(n) < 0.5, 0.3, 0.2)
    perm = rng.permutation(n)
    a0[perm[:TOP]] = 1.0 - (np.arange(TOP) + 1) * 2.0 ** -12
    special = [np.nan, -np.nan, np.inf, -np.inf, 3e160, 1e150, -1e150, -4e149, 1e100, -2.5]
    a0[perm[TOP:TOP + len(special)]] = special
    return np.stack([a0, np.zeros(n)], axis=1)


def first_round(db, n):
    """plants round_avg; returns the scores of a first round, its numbers in descending order and the two values of the body"""
    db.write_avg(round_avg(n), np.ones((n, 2), dtype=np.int32))
    scores = np.array(db.query_round(None, [1.0, 0.0]).scores)
    desc = np.sort(scores[~np.isnan(scores)])[::-1]
    body = np.unique(desc[TOP:][desc[TOP:] > 0])
    assert np.unique(desc[:TOP]).size == TOP and desc[TOP - 1] > desc[TOP] and body.size == 2 and body[1] == desc[TOP] and 0.25 < body[1] < 0.35
    assert np.isnan(scores).sum() == 2 and (scores == -np.inf).sum() == 3 and (scores < -1e149).sum() == 6 and np.nanmin(scores) == -np.inf
    return scores, desc, float(body[1]), float(body[0])


@pytest.mark.parametrize("n", [2049, rc.SMALL_N, BIG_N, 524289])
def test_one_call_round_at_the_prefix_and_past_it(vqa, n):
    """query_round(None, weights, band): bands cut from the first round's own scores so that the match list, then the near list, holds
    1023, 1024 and 1025 rows -- inside the 1024-row prefix, filling it, and past it (the fetch) -- then both lists past it."""
    db = vqa.FeatureDB(n, 2, 1, 4)
    scores, desc, hi, lo = first_round(db, n)
    bands = []
    for c in (1023, 1024, 1025):
        bands += [(c, 5, desc[c - 1], desc[c + 4]), (5, c, desc[4], desc[c + 4])]
    n_hi, n_lo = int((scores == hi).sum()), int((scores == lo).sum())
    bands += [(1025, TOP - 1025 + n_hi, desc[1024], hi), (TOP + n_hi, n_lo, hi, lo), (n - 2, 0, -np.inf, -np.inf), (0, 0, np.nan, 0.5)]
    for n_match, n_near, th, lower in bands:
        r = db.query_round(None, [1.0, 0.0], (th, lower))
        own = np.array(r.scores)
        assert same_bits(own, scores)
        want = np_select(own, th, lower)
        assert (len(r.match_rows), len(r.near_rows)) == (n_match, n_near) == (want[0].size, want[1].size), (n, th, lower)
        assert same_partition((np.array(r.match_rows), np.array(r.near_rows), r.near_argmax), want), (n, n_match, n_near)
    db.close()


# ------------------------------------------------------------------------------------------------------------------- between the two calls
class _WatchedLock:
    """db.lock, saying when a thread other than ``main`` arrives at it and whether ``main`` holds it"""

    def __init__(self, inner, main):
        self.inner, self.main, self.main_depth, self.arrived = inner, main, 0, threading.Event()

    def acquire(self, *args, **kwargs):
        if threading.get_ident() != self.main:
            self.arrived.set()
        got = self.inner.acquire(*args, **kwargs)
        if got and threading.get_ident() == self.main:
            self.main_depth += 1
        return got

    def release(self):
        if threading.get_ident() == self.main:
            self.main_depth -= 1
        self.inner.release()

    def __enter__(self):
        self.acquire()
        return self

    def __exit__(self, *exc):
        self.release()


@pytest.mark.parametrize("intruder", ["select", "topk", "round"])
def test_nothing_comes_between_a_round_and_its_fetch(vqa, monkeypatch, intruder):
    """A round whose near list outgrows the prefix is vq_db_query_round, then vq_db_select_fetch.  Exactly there -- the library call
    of the fetch is held back -- another thread asks the same handle for a selection with shorter lists, a radix top-k (which
    invalidates the lists) or a round under another band.  The fetch goes on once the intruder is through, or once it stands at
    the lock this round holds (it cannot get further however long one waits); 2 s bound the wait.  Both get their own results."""
    fdb = sys.modules[vqa.FeatureDB.__module__]
    n = 20000
    db = vqa.FeatureDB(n, 2, 1, 4)
    scores, desc, _hi, _lo = first_round(db, n)
    main = threading.get_ident()
    db.lock = lock = _WatchedLock(db.lock, main)
    weights = [1.0, 0.0]
    actions = {"select": lambda: db.select(desc[2], desc[6]),
               "topk": lambda: db.topk(5000),
               "round": lambda: db.query_round(None, weights, (0.3, 0.2))}
    state = {"thread": None, "result": None, "error": None}
    done = threading.Event()

    def run():
        try:
            state["result"] = actions[intruder]()
        except BaseException as e:                             # noqa: BLE001 -- reported by the main thread
            state["error"] = e
        finally:
            done.set()
    real = fdb.call

    def call(name, *args):
        if name == "vq_db_select_fetch" and threading.get_ident() == main and state["thread"] is None:
            state["thread"] = threading.Thread(target=run, daemon=True)
            state["thread"].start()
            deadline = time.monotonic() + 2.0
            while not (done.is_set() or (lock.arrived.is_set() and lock.main_depth > 0)) and time.monotonic() < deadline:
                done.wait(0.001)
        return real(name, *args)
    monkeypatch.setattr(fdb, "call", call)
    th, lower = desc[4], 0.25
    try:
        r = db.query_round(None, weights, (th, lower))
    finally:
        monkeypatch.setattr(fdb, "call", real)
        if state["thread"] is not None:
            state["thread"].join(10.0)
    assert state["thread"] is not None, "the round did not take the fetch path"
    assert not state["thread"].is_alive(), "the intruder never returned"
    assert state["error"] is None, state["error"]
    own = np.array(r.scores)
    want = np_select(own, th, lower)
    assert want[1].size > 1024 and same_bits(own, scores)
    assert same_partition((np.array(r.match_rows), np.array(r.near_rows), r.near_argmax), want), \
        "the round's lists are not those of its own band: %d match rows, %d near rows" % (len(r.match_rows), len(r.near_rows))
    got = state["result"]
    if intruder == "select":
        assert same_partition(got, np_select(scores, desc[2], desc[6])) and (len(got[0]), len(got[1])) == (3, 4)
    elif intruder == "topk":
        rows, vals = np_topk(scores, 5000)
        assert np.array_equal(got[0], rows) and same_bits(np.array(got[1]), vals)
    else:
        assert same_bits(np.array(got.scores), scores)
        assert same_partition((np.array(got.match_rows), np.array(got.near_rows), got.near_argmax), np_select(scores, 0.3, 0.2))
    db.close()
