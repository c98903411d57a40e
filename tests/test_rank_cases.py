"""CPU: the case table of tests/_rank_cases.py can tell a wrong ranking kernel from a right one.

Every family meets its own conditions at every size; what a size cannot hold is pinned; and nine deliberately wrong numpy rankers are
run over the table, each of which must disagree with the oracle (np_topk / np_select of tests/_search_set_cases.py) on the family and
size named in its entry.  tests/test_rank_hard_gpu.py walks the same table (rows_of / bands_of / ks_of) on the device."""
import numpy as np
import pytest

import _rank_cases as rc
from _search_set_cases import np_select, np_topk, same_bits

CPU_SIZES = [n for n in rc.SIZES if n <= 40001]           # the mutants and the digit walk run here; the conditions run at every size


def test_order_key_round_trip_and_order():
    bag = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e300, -1e300, 0.8, np.nextafter(0.8, 1), np.nextafter(0.8, 0), 1.0,
                    np.nextafter(1.0, 2), np.nextafter(1.0, 0), -0.5, 2.5, np.nan, -np.nan])
    key = rc.order_key(bag)
    assert key[0] == key[1] == np.uint64(1) << np.uint64(63) and key[-1] == key[-2] == 0
    assert key[3] == rc.KEY_MIN and key[2] == rc.KEY_MAX
    back = rc.from_key(key[2:-2])
    assert same_bits(back, bag[2:-2])
    assert same_bits(rc.from_key(key[:2]), np.array([0.0, 0.0]))
    rows, _vals = np_topk(bag, bag.size)
    by_key = np.lexsort((np.arange(bag.size), ~key))                         # descending key, ties by position
    assert np.array_equal(rows, by_key[:rows.size])
    # keys outside [KEY_MIN, KEY_MAX] invert to NaNs: top byte 0 is -inf or below -2^1009, top byte 255 is +inf or above 2^1009
    assert np.isnan(rc.from_key(np.array([rc.KEY_MIN - 1, rc.KEY_MAX + 1, 1], dtype=np.uint64))).all()
    low, high = rc.from_key(np.array([rc.KEY_MIN, 0x00FFFFFFFFFFFFFF, 0xFF00000000000000, rc.KEY_MAX], dtype=np.uint64)).reshape(2, 2)
    assert low[0] == -np.inf and low[1] <= -2.0 ** 1009 and high[0] >= 2.0 ** 1009 and high[1] == np.inf


@pytest.mark.parametrize("n", rc.SIZES)
def test_every_family_holds_what_its_name_says(n):
    rows = {(r.family, r.variant): r.scores for r in rc.rows_of(n)}
    again = {(r.family, r.variant): r.scores for r in rc.rows_of(n)}
    assert all(same_bits(rows[k], again[k]) for k in rows)                   # deterministic per (family, n)
    for (fam, _v), s in rows.items():
        if fam not in ("uniform3", "all_nan", "one_number", "signs"):
            assert not np.isnan(s).any(), (fam, n)                           # no NaN that was not asked for
    assert np.isnan(rows[("all_nan", "nan")]).all() and (rows[("all_equal", "0.8")] == 0.8).all()
    u = rows[("uniform3", "plain")]
    assert (1 <= np.isnan(u).sum() <= 3 if n > 10 else not np.isnan(u).any()) and (np.round(u[~np.isnan(u)], 3) == u[~np.isnan(u)]).all()
    for name, pos in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        if ("one_number", name) in rows:
            s = rows[("one_number", name)]
            assert np.flatnonzero(~np.isnan(s)).tolist() == [pos]
    assert sorted({0, n // 2, n - 1}) == sorted(int(np.flatnonzero(~np.isnan(s))[0]) for (f, _v), s in rows.items() if f == "one_number")
    for name, _f in rc.TWO_RUN_CUTS:
        c = rc.two_run_cut(name, n)
        assert (c is not None) == (("two_runs", name) in rows)
        if c is not None:                                                    # the run really ends at the boundary it names
            s = rows[("two_runs", name)]
            assert (s[:c] == 0.8).all() and (s[c:] == 0.75).all() and 0 < c < n
            assert c == {"2047": 2047, "2048": 2048, "2049": 2049, "half": n // 2, "last": n - 1}[name]
    mixed, few = rows[("signs", "mixed")], rows[("signs", "few_above_one")]
    if n >= 1023:
        nan = np.isnan(mixed)
        assert abs(int(nan.sum()) - n // 3) <= 1 and (np.signbit(mixed) & nan).any() and (~np.signbit(mixed) & nan).any()
        zero = mixed == 0.0
        assert (zero & np.signbit(mixed)).sum() >= 100 and (zero & ~np.signbit(mixed)).sum() >= 100
        assert (mixed == np.inf).any() and (mixed == -np.inf).any() and (mixed[~nan] < 0).any() and (mixed[~nan] > 1).any()
        tiny = (mixed != 0) & (np.abs(mixed) < 2.2250738585072014e-308)
        assert (tiny & (mixed > 0)).any() and (tiny & (mixed < 0)).any()
        assert np.unique(few).size <= 64 and (few > 1).mean() > 0.5 and not np.isnan(few).any()
    ladder, last = rows[("digit_ladder", "ladder")], rows[("digit_ladder", "last_byte")]
    key = rc.order_key(ladder)
    assert same_bits(rc.from_key(key), ladder) and np.isfinite(ladder).all()
    if n >= 1023:                                                            # every digit at every pass, under the shared prefix
        for p in range(8):
            shift = 56 - 8 * p
            under = key[(key >> np.uint64(shift + 8)) == np.uint64(rc.ladder_prefix(p) >> (shift + 8))] if p else key
            digits = set(((under >> np.uint64(shift)) & np.uint64(255)).tolist())
            assert set(rc.LADDER_DIGITS) <= digits, (p, sorted(set(rc.LADDER_DIGITS) - digits))
        ks = rc.ladder_ks(ladder)
        order = np_topk(ladder, n)[0]
        assert set(ks) == {(p, d) for p in range(8) for d in rc.LADDER_DIGITS} and len(set(ks.values())) >= 72
        for (p, d), k in ks.items():                                         # the k-th best key has digit d under the prefix of pass p
            kth = int(key[order[k - 1]])
            assert (kth >> (56 - 8 * p)) & 255 == d and (p == 0 or kth >> (64 - 8 * p) == rc.ladder_prefix(p) >> (64 - 8 * p)), (p, d, k)
    lk = rc.order_key(last)
    assert ((lk >> np.uint64(8)) == (lk[0] >> np.uint64(8))).all() and np.array_equal(lk & np.uint64(255), np.arange(n, dtype=np.uint64) % np.uint64(256))
    assert np.isfinite(last).all()
    nb = rows[("band_neighbours", "default_band")]
    want = {0.8, np.nextafter(0.8, np.inf), np.nextafter(0.8, -np.inf), 0.73, np.nextafter(0.73, np.inf), np.nextafter(0.73, -np.inf), 0.5}
    assert set(nb.tolist()) <= want and (n < 7 or set(nb.tolist()) == want)
    up, down = rows[("ramp_up", "up")], rows[("ramp_down", "down")]
    assert (np.diff(up) > 0).all() and (np.diff(down) < 0).all()
    assert np.array_equal(np_topk(up, min(5, n))[0], np.arange(n)[::-1][:5]) and np.array_equal(np_topk(down, min(5, n))[0], np.arange(n)[:5])
    for name, pair in rc.near_max_pairs(n).items():
        assert (pair is not None) == (("near_max_ties", name) in rows)
        if pair is not None:
            s = rows[("near_max_ties", name)]
            match, near, arg = np_select(s, rc.TH, rc.LOWER)
            assert arg == pair[0] and s[pair[0]] == s[pair[1]] == s[near].max() and pair[1] in near and (match.size or n == 2)
            assert np.flatnonzero(s == s[arg]).tolist() == sorted(pair)
    for b, name in ((0, "block_0"), (255, "block_255"), (256, "block_256")):
        pair = rc.near_max_pairs(n)[name]
        if pair is not None:                                                 # last row of block b | first row of block b + 1
            assert pair[0] // rc.SEL_CHUNK == b and pair[1] // rc.SEL_CHUNK == b + 1 and pair[1] == pair[0] + 1


def test_only_what_a_size_cannot_hold_is_skipped():
    """Pinned independently of the builders: which (family, variant) a size lacks, and which band a row lacks."""
    for n in rc.SIZES:
        want = set()
        want |= {("one_number", "middle")} if n // 2 == 0 else set()                 # a position named twice is planted once
        want |= {("one_number", "last")} if n - 1 in (0, n // 2) else set()
        cuts = {"2047": 2047, "2048": 2048, "2049": 2049}
        want |= {("two_runs", nm) for nm, c in cuts.items() if c >= n}
        want |= {("two_runs", "half")} if n < 2 or n // 2 in cuts.values() else set()
        want |= {("two_runs", "last")} if n < 2 or n - 1 in list(cuts.values()) + [n // 2] else set()
        want |= {("near_max_ties", "block_%d" % b) for b in (0, 255, 256) if 2048 * (b + 1) >= n}
        want |= {("near_max_ties", "thread_run")} if n <= 19 else set()
        want |= {("near_max_ties", "wave")} if n <= 512 else set()
        want |= {("near_max_ties", "last_rows")} if n < 2 else set()
        assert set(rc.skipped_of(n)) == want, (n, sorted(set(rc.skipped_of(n)) ^ want))
        assert {r.family for r in rc.rows_of(n)} == set(rc.families_at(n))
        assert n < 2 or rc.families_at(n) == rc.FAMILIES                     # from two rows on every family is there
    assert rc.near_max_pairs(1048581)["block_256"] is not None and rc.near_max_pairs(524289)["last_rows"] == (524287, 524288)
    for n in CPU_SIZES:
        for r in rc.rows_of(n):
            lack = set(rc.skipped_bands(r.scores))
            want = ({"planted"} if np.isnan(r.scores).all() else set()) | (set() if rc.has_both_zeros(r.scores) else {"plus_zero", "minus_zero"})
            assert lack == want, (r.family, r.variant, n)
            assert (r.family, r.variant) != ("signs", "mixed") or n < 16 or not lack
            ks = rc.ks_of(r.scores)
            nv = int((~np.isnan(r.scores)).sum())
            assert {1, min(2, n), n, min(max(nv, 1), n), min(1024, n), min(1025, n)} <= set(ks) and all(1 <= k <= n for k in ks)


@pytest.mark.parametrize("n", CPU_SIZES)
def test_the_digit_walk_restated_in_numpy_is_the_oracle(n):
    """radix_topk (the kernels' algorithm: eight passes, the walk down to bin 0, the compaction) == np_topk on every row and k."""
    for r in rc.rows_of(n):
        ks = rc.ks_of(r.scores) if n <= 2049 or r.family in ("digit_ladder", "signs") else rc.ks_of(r.scores)[:4]
        for k in ks:
            rows, vals = rc.radix_topk(r.scores, k)
            want_rows, want_vals = np_topk(r.scores, k)
            assert np.array_equal(rows, want_rows) and same_bits(vals, want_vals), (r.family, r.variant, n, k)


# ------------------------------------------------------------------------------------------------------------------------- mutants
def _topk_by(sort_value, scores, k, keep=None, tie=1):
    v = np.asarray(scores)
    idx = np.flatnonzero(~np.isnan(v)) if keep is None else keep
    order = idx[np.lexsort((tie * idx, -sort_value[idx]))][:k]
    return order.astype(np.int64), v[order]


def m_ties_descending_position(s, k):
    return _topk_by(s, s, k, tie=-1)


def m_raw_bits_zero(s, k):
    """-0.0 below +0.0: the key without the fold of the zeros, compared as integers"""
    b = np.ascontiguousarray(s).view(np.uint64)
    key = np.where((b >> np.uint64(63)) != 0, ~b, b | (np.uint64(1) << np.uint64(63)))
    idx = np.flatnonzero(~np.isnan(s))
    order = idx[np.lexsort((idx, np.uint64(0xFFFFFFFFFFFFFFFF) - key[idx]))][:k]
    return order.astype(np.int64), s[order]


def m_nan_smallest(s, k):
    return _topk_by(np.where(np.isnan(s), -np.inf, s), s, k, keep=np.arange(s.size))


def m_top_56_bits(s, k):
    """a radix select that stops one pass early: keys that agree on their top seven bytes count as tied"""
    idx = np.flatnonzero(~np.isnan(s))
    order = idx[np.lexsort((idx, ~(rc.order_key(s)[idx] >> np.uint64(8))))][:k]
    return order.astype(np.int64), s[order]


def m_float32(s, k):
    with np.errstate(over="ignore"):
        return _topk_by(s.astype(np.float32).astype(np.float64), s, k)


def m_never_bin_0(s, k):
    return rc.radix_topk(s, k, lowest_bin=1)


def m_strictly_above_threshold(s, th, lower):
    with np.errstate(invalid="ignore"):
        match, near = np.flatnonzero(s > th), np.flatnonzero((lower <= s) & (s < th))
    return match, near, (int(near[np.argmax(s[near])]) if near.size else -1)


def m_near_upper_edge_inclusive(s, th, lower):
    with np.errstate(invalid="ignore"):
        match, near = np.flatnonzero(s >= th), np.flatnonzero((lower <= s) & (s <= th))
    return match, near, (int(near[np.argmax(s[near])]) if near.size else -1)


def m_last_near_maximum(s, th, lower):
    match, near, _arg = np_select(s, th, lower)
    return match, near, (int(near[near.size - 1 - np.argmax(s[near][::-1])]) if near.size else -1)


# mutant -> (kind, ranker, the family and size that must expose it)
MUTANTS = {
    "ties broken by descending position": ("topk", m_ties_descending_position, "all_equal", 64),
    "> instead of >= at the threshold": ("select", m_strictly_above_threshold, "all_equal", 64),
    "the near band's upper edge inclusive": ("select", m_near_upper_edge_inclusive, "band_neighbours", 1023),
    "-0.0 ranked below +0.0": ("topk", m_raw_bits_zero, "signs", 1023),
    "NaN ranked as the smallest number": ("topk", m_nan_smallest, "one_number", 63),
    "keys compared on their top 56 bits": ("topk", m_top_56_bits, "digit_ladder", 1023),
    "scores compared after rounding to float32": ("topk", m_float32, "band_neighbours", 1023),
    "a near arg-max that keeps the last maximum": ("select", m_last_near_maximum, "near_max_ties", 1025),
    "a digit walk that never takes bin 0": ("topk", m_never_bin_0, "digit_ladder", 1023),
}


def _first_disagreement(kind, ranker, row):
    s = row.scores
    if kind == "topk":
        for k in rc.ks_of(s):
            got, want = ranker(s, k), np_topk(s, k)
            if not (np.array_equal(got[0], want[0]) and same_bits(np.asarray(got[1]), np.asarray(want[1]))):
                return "k = %d" % k
    else:
        for name, th, lower in rc.bands_of(s):
            got, want = ranker(s, th, lower), np_select(s, th, lower)
            if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]):
                return "band %s (%r, %r)" % (name, th, lower)
    return None


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_wrong_ranker_is_caught(name):
    kind, ranker, family, n = MUTANTS[name]
    caught = [(r.variant, _first_disagreement(kind, ranker, r)) for r in rc.rows_of(n, (family,))]
    caught = [(v, where) for v, where in caught if where]
    assert caught, "%s: not exposed by family %s at n = %d" % (name, family, n)
    print("mutant %-45s caught by %s/%s, n = %d, %s" % (name, family, caught[0][0], n, caught[0][1]))
