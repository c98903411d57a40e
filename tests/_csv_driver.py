"""Shared by the feature-CSV reader's tests: the sanitizer build of its host code (tests/sanitize_csv, a stand-alone program under
ASan + UBSan, built once per test session) and the hard inputs every layer is held against."""
import atexit
import functools
import os
import shutil
import struct
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINDINGS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: ")

# rounding boundaries, subnormals, overflow and underflow, the forms of the grammar: every one must come out as float() reads it
HARD = ["9007199254740993", "9007199254740995", "0.1", "5e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
        "4.9406564584124654e-324", "2.2250738585072011e-308", "2.2250738585072014e-308", "1.7976931348623157e308",
        "1.7976931348623159e308", "1e22", "1e23", "1e-400", "1e400", "9223372036854775807", "-0.0", ".5", "5.", "1E5"]
# what the device hands to the host: more than 19 digits, blanks, the words
SLOW = ["12345678901234567890", " 1.5", "inf", "NaN"]


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@functools.lru_cache(maxsize=None)
def driver() -> str:
    out = tempfile.mkdtemp(prefix="csvsan_")
    atexit.register(shutil.rmtree, out, True)
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "sanitize_csv"), "OUT=" + out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return os.path.join(out, "csv_driver_asan")


def run(*args) -> str:
    """The driver's standard output; a sanitizer finding or a non-zero exit fails the test that asked."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver()] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert r.returncode == 0 and not any(tag in r.stdout for tag in FINDINGS), r.stdout[-4000:]
    return r.stdout


def tally(text: str) -> dict:
    """'fields N decided N undecided N ask_host N mismatches N' -> dict"""
    words = text.strip().split("\n")[-1].split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
