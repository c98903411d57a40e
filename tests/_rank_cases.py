"""Test infrastructure, no GPU: the table of hard score rows for the one-query ranking kernels (select_small / select_count / scan /
scatter, topk_small / topk_hist / topk_pick, gather_scores in csrc/vq_rank.hip, the shared steps in csrc/vq_select.h).

A case is (family, variant, n) -> a float64 row, deterministic per (family, n); ``bands_of`` and ``ks_of`` give the (threshold, lower)
bands and the k values a row is ranked under.  ``skipped_of`` / ``skipped_bands`` list what a size cannot hold BY CONSTRUCTION (a tie
run needs two rows, a boundary at 2048 needs more rows than that, a planted band needs a number in the row); tests/test_rank_cases.py
pins those lists, so a case cannot drop out quietly.  The oracle stays ``np_topk`` / ``np_select`` / ``np_min_score`` of
tests/_search_set_cases.py; ``radix_topk`` restates the kernels' MSB-first digit walk in numpy (test_rank_cases.py checks it against
the oracle and builds a mutant from it)."""
from collections import namedtuple

import numpy as np

from _search_set_cases import tie_ks

SEL_CHUNK = 2048                  # csrc/vq_select.h: rows per block of the three-pass partition
SMALL_N = 16384                   # kSelSmallN = kTopkSmallN: the one-workgroup forms end here
SMALL_K = 1024                    # kTopkSmallK
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 40001, 524287, 524288, 524289, 1048581)
FAMILIES = ("uniform3", "all_equal", "all_nan", "one_number", "two_runs", "signs", "digit_ladder", "band_neighbours", "ramp_up", "ramp_down",
            "near_max_ties")
TH, LOWER = 0.8, 0.73             # the default band; band_neighbours and near_max_ties are built around it

_TOP = np.uint64(1) << np.uint64(63)
KEY_MIN, KEY_MAX = 0x000FFFFFFFFFFFFF, 0xFFF0000000000000       # -inf and +inf: keys outside invert to NaNs
LADDER_DIGITS = (0, 1, 3, 4, 127, 128, 251, 252, 254, 255)       # bin 0, bin 255, both sides of radix_pick_wave's four bins per lane
LADDER_BASE = (0x9A, 0x5C, 0x33, 0xC7, 0x6E, 0x81, 0x2B, 0xE2)   # the prefix the groups share: no byte of it is a ladder digit

Row = namedtuple("Row", "family variant n scores")


# ------------------------------------------------------------------------------------------------------------------------- keys
def order_key(v):
    """csrc/vq_select.h order_key: NaN -> 0, -0 -> +0, a negative value -> ~bits, anything else -> bits | 1 << 63"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.uint64)
    b = np.where(v == 0.0, np.uint64(0), b)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | _TOP)
    return np.where(np.isnan(v), np.uint64(0), k).astype(np.uint64)


def from_key(k):
    """the score with that key (the inverse of order_key on [KEY_MIN, KEY_MAX] but for the key of -0, which order_key never gives)"""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k ^ _TOP, ~k).astype(np.uint64).view(np.float64)


def key_is_a_number(k):
    k = np.asarray(k, dtype=np.uint64)
    return (k >= np.uint64(KEY_MIN)) & (k <= np.uint64(KEY_MAX)) & (k != np.uint64(0x7FFFFFFFFFFFFFFF))


def radix_topk(scores, k, lowest_bin=0):
    """topk_hist_kernel / topk_pick_kernel / the compaction with limit1, in numpy: eight passes from the top byte down, the walk from
    bin 255 to ``lowest_bin`` (which takes what is left), then keys above the pivot and the first ``need`` that tie with it, sorted by
    descending score and ascending position.  lowest_bin = 0 is the kernels' algorithm."""
    v = np.asarray(scores, dtype=np.float64)
    key = order_key(v)
    live = key != 0
    prefix, need = 0, int(k)
    for p in range(8):
        shift = 56 - 8 * p
        mask = 0 if p == 0 else (0xFFFFFFFFFFFFFFFF << (shift + 8)) & 0xFFFFFFFFFFFFFFFF
        sel = live & ((key & np.uint64(mask)) == np.uint64(prefix))
        hist = np.bincount(((key[sel] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        b = 255
        while b > lowest_bin:
            if hist[b] >= need:
                break
            need -= int(hist[b])
            b -= 1
        prefix |= b << shift
    gt = np.flatnonzero(key > np.uint64(prefix))
    eq = np.flatnonzero(live & (key == np.uint64(prefix)))[:max(need, 0)]
    rows = np.concatenate([gt, eq])
    rows = rows[np.lexsort((rows, -v[rows]))][:int(k)]
    return rows.astype(np.int64), v[rows]


# ------------------------------------------------------------------------------------------------------------------------- rows
def _rng(family, n):
    return np.random.default_rng([FAMILIES.index(family), n])


def _uniform3(n):
    rng = _rng("uniform3", n)
    row = np.round(rng.random(n), 3)
    if n > 10:
        row[rng.integers(0, n, 3)] = np.nan
        row[rng.integers(0, n, 3)] = -0.5
    return [("plain", row)]


def _all_equal(n):
    return [("0.8", np.full(n, TH))]


def _all_nan(n):
    return [("nan", np.full(n, np.nan))]


def _one_number(n):
    out = []
    for name, pos in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        if pos not in [p for _n, p in out]:
            out.append((name, pos))
    rows = []
    for name, pos in out:
        row = np.full(n, np.nan)
        row[pos] = 0.75
        rows.append((name, row))
    return rows


TWO_RUN_CUTS = (("2047", lambda n: 2047), ("2048", lambda n: 2048), ("2049", lambda n: 2049), ("half", lambda n: n // 2), ("last", lambda n: n - 1))


def two_run_cut(name, n):
    """the first row of the second run, or None where the size cannot hold it (a run needs a row on either side) or an earlier cut is it"""
    seen = []
    for nm, f in TWO_RUN_CUTS:
        c = f(n)
        ok = 0 < c < n and c not in seen
        if ok:
            seen.append(c)
        if nm == name:
            return c if ok else None
    raise KeyError(name)


def _two_runs(n):
    rows = []
    for name, _f in TWO_RUN_CUTS:
        c = two_run_cut(name, n)
        if c is not None:
            row = np.full(n, 0.75)
            row[:c] = TH
            rows.append((name, row))
    return rows


def _signs(n):
    """what tests/test_batch_topk_gpu.py::test_signs plants: both signs, both zeros, both infinities, NaNs of both signs over a third of
    the row, subnormals, values above 1; and a row of few distinct values, most above 1"""
    rng = _rng("signs", n)
    row = rng.standard_normal(n) * np.resize(np.array([1.0, 1e-3, 50.0, 1e300, 1e-310, 2.0]), n)
    perm = rng.permutation(n)
    at = 0

    def take(count):
        nonlocal at
        idx = perm[at:at + count]
        at += count
        return idx
    nan_rows = take(n // 3)
    row[nan_rows] = np.nan
    row[nan_rows[::7]] = -np.nan
    row[take(n // 8)] = 0.0
    row[take(n // 8)] = -0.0
    row[take(max(n // 50, 1 if n >= 16 else 0))] = np.inf
    row[take(max(n // 50, 1 if n >= 16 else 0))] = -np.inf
    sub = take(n // 20)
    row[sub] = 5e-324 * rng.integers(1, 1000, sub.size) * np.where(np.arange(sub.size) % 2, -1.0, 1.0)
    big = take(n // 10)
    row[big] = 1.0 + np.abs(rng.standard_normal(big.size))
    few = np.round(rng.standard_normal(n) * 4) / 4 + 1.5
    return [("mixed", row), ("few_above_one", few)]


def ladder_prefix(p):
    """the top p bytes of LADDER_BASE as the high bits of a key"""
    out = 0
    for i in range(p):
        out |= LADDER_BASE[i] << (56 - 8 * i)
    return out


def _digit_ladder(n):
    """ladder: for every pass p a group of keys that agrees with LADDER_BASE on the top p bytes and has byte p in LADDER_DIGITS, random
    below; at most 48 rows per (pass, digit), spread over the whole row, and every other row a key with top byte 0 (finite, below
    -2^1009: pass 0's bin 0).  last_byte: from_key(base + i mod 256): every top-k is decided in pass 7."""
    rng = _rng("digit_ladder", n)
    per = min(max(n // 80, 1), 48)
    keys = []
    for p in range(8):
        shift = 56 - 8 * p
        for d in LADDER_DIGITS:
            low = rng.integers(0, 1 << shift, 4 * per + 8, dtype=np.uint64) if shift else np.zeros(4 * per + 8, dtype=np.uint64)
            cand = np.uint64(ladder_prefix(p) | (d << shift)) | low
            cand = cand[key_is_a_number(cand)]                         # a key that inverts to a NaN is dropped, not planted
            keys.append(cand[:per])
    keys = np.concatenate(keys)
    keys = keys[rng.permutation(keys.size)][:n]
    filler = rng.integers(KEY_MIN, 1 << 56, n, dtype=np.uint64)        # top byte 0
    at = np.sort(rng.choice(n, keys.size, replace=False))
    filler[at] = keys
    ladder = from_key(filler)
    base = np.uint64(ladder_prefix(7))
    last = from_key(base + (np.arange(n, dtype=np.uint64) % np.uint64(256)))
    for row in (ladder, last):
        assert not np.isnan(row).any(), "the ladder planted a NaN it did not ask for"
    return [("ladder", ladder), ("last_byte", last)]


def ladder_groups(scores):
    """{(pass, digit): rows} of a ladder row: the rows whose key agrees with LADDER_BASE on the top ``pass`` bytes and has ``digit`` next"""
    key = order_key(scores)
    out = {}
    for p in range(8):
        shift = 56 - 8 * p
        under = (key >> np.uint64(shift + 8)) == np.uint64(ladder_prefix(p) >> (shift + 8)) if p else np.ones(key.size, dtype=bool)
        digit = (key >> np.uint64(shift)) & np.uint64(255)
        for d in LADDER_DIGITS:
            rows = np.flatnonzero(under & (digit == np.uint64(d)))
            if rows.size:
                out[(p, d)] = rows
    return out


def ladder_ks(scores):
    """{(pass, digit): k}: a k whose k-th best key lies in the middle of that group, so that the walk of pass ``pass`` stops in bin
    ``digit`` -- every digit of LADDER_DIGITS decides at every pass"""
    rank = np.empty(scores.size, dtype=np.int64)
    rank[np.lexsort((np.arange(scores.size), ~order_key(scores)))] = np.arange(scores.size)
    return {g: int(np.sort(rank[rows])[rows.size // 2]) + 1 for g, rows in ladder_groups(scores).items()}


def _band_neighbours(n):
    pattern = np.array([TH, np.nextafter(TH, np.inf), np.nextafter(TH, -np.inf), LOWER, np.nextafter(LOWER, np.inf), np.nextafter(LOWER, -np.inf), 0.5])
    return [("default_band", np.resize(pattern, n))]


def _ramp_up(n):
    return [("up", -0.25 + 1.5 * np.arange(n) / n)]


def _ramp_down(n):
    return [("down", (-0.25 + 1.5 * np.arange(n) / n)[::-1].copy())]


def near_max_pairs(n):
    """variant -> the two rows that hold the near band's maximum (the first must win), or None where the size cannot hold them"""
    out = {}
    for b in (0, 255, 256):
        hi = SEL_CHUNK * (b + 1)                                       # last row of block b | first row of block b + 1
        out["block_%d" % b] = (hi - 1, hi) if hi < n else None
    out["thread_run"] = (16, 19) if n > 19 else None                   # inside one run of SEL_ITEMS = 8 consecutive rows
    out["wave"] = (511, 512) if n > 512 else None                      # 64 threads x 8 rows: a wave boundary of the three-pass form
    out["last_rows"] = (n - 2, n - 1) if n >= 2 else None              # the ragged last block
    return out


def _near_max_ties(n):
    rng = _rng("near_max_ties", n)
    base = rng.random(n) * 0.7                                         # below the near band
    base[::97] = 0.9                                                   # some matches
    base[5::53] = 0.75                                                 # a near band with more than its maximum in it
    rows = []
    for name, pair in near_max_pairs(n).items():
        if pair is not None:
            row = base.copy()
            row[list(pair)] = 0.79
            rows.append((name, row))
    return rows


_BUILDERS = {"uniform3": _uniform3, "all_equal": _all_equal, "all_nan": _all_nan, "one_number": _one_number, "two_runs": _two_runs, "signs": _signs,
             "digit_ladder": _digit_ladder, "band_neighbours": _band_neighbours, "ramp_up": _ramp_up, "ramp_down": _ramp_down,
             "near_max_ties": _near_max_ties}
VARIANTS = {"uniform3": ("plain",), "all_equal": ("0.8",), "all_nan": ("nan",), "one_number": ("first", "middle", "last"),
            "two_runs": tuple(nm for nm, _f in TWO_RUN_CUTS), "signs": ("mixed", "few_above_one"), "digit_ladder": ("ladder", "last_byte"),
            "band_neighbours": ("default_band",), "ramp_up": ("up",), "ramp_down": ("down",),
            "near_max_ties": ("block_0", "block_255", "block_256", "thread_run", "wave", "last_rows")}


def families_at(n):
    """the families with a row of size n without building one: a single row holds neither two runs nor a tied pair (pinned by
    tests/test_rank_cases.py against rows_of)"""
    return FAMILIES if n >= 2 else tuple(f for f in FAMILIES if f not in ("two_runs", "near_max_ties"))


def rows_of(n, families=FAMILIES):
    """every Row of size n, family by family"""
    out = []
    for fam in families:
        for variant, scores in _BUILDERS[fam](n):
            assert scores.shape == (n,) and scores.dtype == np.float64 and variant in VARIANTS[fam]
            out.append(Row(fam, variant, n, scores))
    return out


def skipped_of(n, families=FAMILIES):
    """the (family, variant) pairs size n cannot hold"""
    have = {(r.family, r.variant) for r in rows_of(n, families)}
    return [(fam, v) for fam in families for v in VARIANTS[fam] if (fam, v) not in have]


# ------------------------------------------------------------------------------------------------------------------------- bands, k
BAND_NAMES = ("default", "planted", "empty", "inverted", "inf_neginf", "all_match", "nan_threshold", "nan_lower", "plus_zero", "minus_zero")


def has_both_zeros(scores):
    z = scores == 0.0
    return bool((z & np.signbit(scores)).any() and (z & ~np.signbit(scores)).any())


def bands_of(scores):
    """[(name, threshold, lower)]: see BAND_NAMES.  ``planted`` takes both edges from the row (>= is inclusive, the near band's upper
    edge exclusive: rows equal to the threshold match, rows equal to lower are near); the two zero bands need a row with both zeros."""
    out = [("default", TH, LOWER)]
    vals = np.unique(scores[~np.isnan(scores)])
    if vals.size:
        out.append(("planted", float(vals[(2 * vals.size) // 3]), float(vals[vals.size // 3])))
    out += [("empty", TH, TH), ("inverted", LOWER, TH), ("inf_neginf", np.inf, -np.inf), ("all_match", -np.inf, -np.inf),
            ("nan_threshold", np.nan, 0.5), ("nan_lower", TH, np.nan)]
    if has_both_zeros(scores):
        out += [("plus_zero", 0.0, -1.0), ("minus_zero", -0.0, -1.0)]
    return out


def skipped_bands(scores):
    return [b for b in BAND_NAMES if b not in [name for name, _t, _l in bands_of(scores)]]


def ks_of(scores):
    """1 and 2; the middle of the best tie run, its end, one past it (tie_ks); SMALL_K and SMALL_K + 1; n_valid - 1, n_valid, n_valid + 1
    and n.  Clamped to [1, n] as FeatureDB.topk clamps, each once, ascending."""
    n = scores.size
    nv = int((~np.isnan(scores)).sum())
    ks = [1, 2, SMALL_K, SMALL_K + 1, nv - 1, nv, nv + 1, n] + tie_ks(scores, n)
    return sorted({min(max(int(k), 1), n) for k in ks})
