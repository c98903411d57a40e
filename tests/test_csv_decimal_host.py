"""CPU: the decimal arithmetic the device loader of feature CSV files shares with the host (csrc/vq_decimal.h), run on the host by the
stand-alone driver of tests/sanitize_csv under ASan + UBSan and held against glibc strtod bit for bit; the host's parser for the
fields the device hands back; the storage conversions against numpy's astype.

Bounds: mismatches 0 (both sides are correctly rounded: there is one right answer).  "Cannot decide" at most 1 field in 10^5 -- the
truncated 128-bit product leaves the rounding open only when 9 + 64 product bits are all ones; on the reference's shipped files and
on random prints it never happened when this was written."""
import glob
import lzma
import os
import struct

import numpy as np

import _csv_driver as cd
from _helpers import GOLDEN


def _random_finite_doubles(rng, n):
    raw = rng.integers(0, 1 << 64, size=n + n // 256 + 64, dtype=np.uint64)
    v = raw.view(np.float64)
    v = v[np.isfinite(v)][:n]
    assert v.size == n
    return v


def test_every_field_of_the_shipped_feature_files(tmp_path):
    paths = []
    for k, src in enumerate(sorted(glob.glob(os.path.join(GOLDEN, "reference_features", "**", "*.csv.xz"), recursive=True))):
        paths.append(str(tmp_path / ("f%d.csv" % k)))
        with lzma.open(src) as f, open(paths[-1], "wb") as g:
            g.write(f.read())
    assert len(paths) == 7
    t = cd.tally(cd.run("csvfields", *paths))
    print(t)
    assert t["fields"] == 651264 and t["mismatches"] == 0 and t["ask_host"] == 0
    assert t["undecided"] <= 6 and t["decided"] == t["fields"] - t["undecided"]


def test_prints_of_random_bit_patterns_over_the_whole_exponent_range(tmp_path):
    v = _random_finite_doubles(np.random.default_rng(20261019), 500000)
    path = str(tmp_path / "prints.txt")
    with open(path, "w") as f:
        f.write("\n".join(repr(x) for x in v.tolist()))
        f.write("\n")
        f.write("\n".join("%.12g" % x for x in v.tolist()))
        f.write("\n")
    t = cd.tally(cd.run("fields", path))
    print(t)
    assert t["fields"] == 1000000 and t["mismatches"] == 0 and t["ask_host"] == 0
    assert t["undecided"] <= t["fields"] // 100000


def test_neighbours_of_float32_means_printed_with_17_digits(tmp_path):
    """Features are means of T float32 blobs (calcSig_wOF.py:82): short binary fractions whose 17-digit prints sit close to rounding
    boundaries of nothing in particular -- and their neighbours one ulp either side print as close to a boundary as a print can."""
    rng = np.random.default_rng(7)
    a = (rng.random((10000, 25)).astype(np.float32) * np.float32(3.0)).astype(np.float64).sum(axis=1) / 25.0
    vals = np.concatenate([a, np.nextafter(a, np.inf), np.nextafter(a, -np.inf)])
    path = str(tmp_path / "means.txt")
    with open(path, "w") as f:
        f.write("\n".join("%.17g" % x for x in vals.tolist()) + "\n")
    t = cd.tally(cd.run("fields", path))
    print(t)
    assert t["fields"] == 30000 and t["mismatches"] == 0 and t["ask_host"] == 0 and t["undecided"] == 0


def test_the_hard_list_and_what_goes_to_the_host():
    out = cd.run("probe", *(cd.HARD + cd.SLOW + ["1_0", "0x10", "", "1e", "١", "1.5 ", "-Infinity", "+.5e1", "- 1"])).strip().split("\n")
    for s, line in zip(cd.HARD, out):
        status, bits, _h, hbits = line.split()
        assert status == "ok" and int(bits, 16) == cd.bits_of(float(s)) and int(hbits, 16) == cd.bits_of(float(s)), (s, line)
    rest = out[len(cd.HARD):]
    for s, line in zip(cd.SLOW, rest):
        status, _bits, _h, hbits = line.split()
        assert status == ("undecided" if s[0] == "1" and len(s) == 20 else "ask_host"), (s, line)
        assert int(hbits, 16) == cd.bits_of(float(s)), (s, line)                 # the host parser gives float()'s bits
    refused = rest[len(cd.SLOW):len(cd.SLOW) + 5]
    assert all(line.split()[0] == "ask_host" and line.endswith("host invalid") for line in refused), refused      # Python takes two of them
    for s, line in zip(["1.5 ", "-Infinity", "+.5e1"], rest[len(cd.SLOW) + 5:]):
        assert int(line.split()[3], 16) == cd.bits_of(float(s)), (s, line)
    assert rest[-1].endswith("host invalid")


def _convert(values):
    values = np.asarray(values, dtype=np.float64)
    got = []
    for k in range(0, values.size, 2000):
        lines = cd.run("convert", *("%016x" % b for b in values[k:k + 2000].view(np.uint64).tolist())).strip().split("\n")
        got.extend(line.split() for line in lines)
    f32 = np.array([int(g[0], 16) for g in got], dtype=np.uint32)
    o32 = np.array([int(g[1]) for g in got], dtype=bool)
    f16 = np.array([int(g[2], 16) for g in got], dtype=np.uint16)
    o16 = np.array([int(g[3]) for g in got], dtype=bool)
    return f32, o32, f16, o16


def test_storage_conversions_round_once_like_numpy():
    rng = np.random.default_rng(3)
    half_tie_through_float = 1.0 + 2.0 ** -11 + 2.0 ** -30      # above the tie between two halves; float drops 2^-30 and makes it a tie
    with np.errstate(over="ignore"):
        assert np.float64(half_tie_through_float).astype(np.float32).astype(np.float16) != np.float64(half_tie_through_float).astype(np.float16)
    named = [65519.999999999993, 65520.0, half_tie_through_float, 2.0 ** -24, 2.0 ** -25, np.nextafter(2.0 ** -25, 1.0), -65520.0, 65504.0,
             0.0, -0.0, np.inf, -np.inf, 3.4028235677973366e38, 3.4028235677973362e38, 1e39, 2.0 ** -149, 2.0 ** -150,
             np.nextafter(2.0 ** -150, 1.0), 2.0 ** -126, 1e-320, 6.103515625e-05, 6.097555160522461e-05]
    scattered = np.concatenate([
        _random_finite_doubles(rng, 2000),
        rng.standard_normal(2000) * 10.0 ** rng.integers(-9, 6, 2000),                       # the range of halves, subnormal halves included
        (rng.integers(0, 1 << 11, 1000) + 0.5) * 2.0 ** rng.integers(-24, 6, 1000),          # exact ties between halves
        (rng.integers(0, 1 << 24, 1000) + 0.5) * 2.0 ** rng.integers(-149, 100, 1000),       # exact ties between floats
        rng.standard_normal(1000) * 10.0 ** rng.integers(-46, -36, 1000),                    # subnormal floats
    ])
    vals = np.concatenate([np.array(named, dtype=np.float64), scattered])
    f32, o32, f16, o16 = _convert(vals)
    with np.errstate(over="ignore", under="ignore"):
        want32 = vals.astype(np.float32)
        want16 = vals.astype(np.float16)
    assert (f32 == want32.view(np.uint32)).all()
    assert (o32 == (np.isinf(want32) & np.isfinite(vals))).all()
    assert (f16 == want16.view(np.uint16)).all()
    assert (o16 == (np.isinf(want16) & np.isfinite(vals))).all()
    assert f16[0] == np.float16(65504.0).view(np.uint16) and not o16[0] and o16[1] and o16[6]       # 65519.99.. -> 65504; +-65520 refused
    assert f16[3] == 1 and f16[4] == 0 and f16[5] == 1                                              # the smallest subnormal half; 2^-25 -> 0
    assert struct.unpack("<e", struct.pack("<H", int(f16[2])))[0] == 1.0 + 2.0 ** -10
