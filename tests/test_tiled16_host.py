"""CPU: what VQ_LAYOUT_TILED16 (the tiled layout of float16 databases) adds outside the kernels.

  * the value: include/vq_amd.h and _lib agree on 3; additive to ABI 12 -- no new exported name; feature_db.LAYOUTS holds the four names;
  * the element-address rule (csrc/vq_tile_index.h) at the unit of halves, U = 8: compiled into a stand-alone host program
    (tests/sanitize/tile16_driver.cc) under AddressSanitizer + UndefinedBehaviorSanitizer -- nothing sanitised is loaded here;
  * ShardedFeatureDB.set_layout over gloo, every rank's database a numpy stand-in: "tiled16" reaches every rank, and the announcement
    carries 3 ("rows", "tiled" and "tiled64" keep 0, 1 and 2);
  * the premise under which tests/test_tiled16_gpu.py compares ranks on the goldens rounded to binary16, checked with the oracle.

The GPU half is tests/test_tiled16_gpu.py."""
import glob
import os
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

from _tiled16_cases import CFG1_BAND, GAP, GOLDENS, MIN_KEPT, cfg1_case16, golden_case16, oracle_scores16, rank_prefix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-query-algorithms_amd", "csrc")
FINDINGS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "SUMMARY: ")


def _declared(header):
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M))


def test_the_value_is_additive_to_abi_12():
    import video_query_algorithms_amd as vqa
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        header = f.read()
    assert re.search(r"^enum\s*\{\s*VQ_LAYOUT_TILED16 = 3\s*\};", header, flags=re.M)
    assert vqa._lib.VQ_LAYOUT_TILED16 == 3
    assert (vqa._lib.VQ_LAYOUT_ROWS, vqa._lib.VQ_LAYOUT_TILED, vqa._lib.VQ_LAYOUT_TILED64) == (0, 1, 2)
    assert re.search(r"#define\s+VQ_ABI_VERSION\s+12\b", header) and vqa.load_library().vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    # no new entry point: the main header still declares 102, and what the library exports is what the headers declare
    assert len(_declared(os.path.join(ROOT, "include", "vq_amd.h"))) == 102 == len(vqa._lib.exported_symbols())
    declared = set().union(*(_declared(h) for h in glob.glob(os.path.join(ROOT, "include", "*.h"))))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", vqa._lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("vq_")}
        assert exported == declared
    assert len(declared) == 130 and not any("tiled" in n or "16" in n for n in declared)


def test_one_table_holds_the_four_names():
    from video_query_algorithms_amd import feature_db, sharded_db
    assert feature_db.LAYOUTS == {"rows": 0, "tiled": 1, "tiled64": 2, "tiled16": 3}
    assert feature_db.LAYOUT_NAMES == {0: "rows", 1: "tiled", 2: "tiled64", 3: "tiled16"}
    assert sharded_db.LAYOUTS is feature_db.LAYOUTS                    # both ends of OP_LAYOUT look names up in the same table
    with pytest.raises(KeyError):
        feature_db.LAYOUTS["tiled128"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tile16") / "tile16_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "tile16_driver.cc"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0 and not any(tag in r.stdout for tag in FINDINGS), r.stdout[-4000:]
    return r.stdout


def test_the_unit_of_halves_is_a_bijection_onto_the_tiles_under_asan_ubsan(driver):
    """U = 8 (tile_unit_of(2), checked by the driver), n in {1, 16, 17, 37} and the largest shape: one to one onto the whole tiles, units
    contiguous, 64 consecutive units 4 k-groups of 16 clips (the driver's own checks), and a few elements against the rule restated
    here."""
    assert _run(driver).strip().endswith("tile16: ok")

    def rule(U, row, NV, v, D, k):
        if U == 0:
            return (row * NV + v) * D + k
        return ((((row >> 4) * NV + v) * (D // U) + k // U) * 16 + (row & 15)) * U + k % U
    rng = np.random.default_rng(16)
    for U in (0, 8):
        for _ in range(8):
            NV, D = int(rng.integers(1, 11)), 1024
            row, v, k = int(rng.integers(0, 3_000_000)), int(rng.integers(0, NV)), int(rng.integers(0, D))      # past 2^31 elements
            assert int(_run(driver, U, row, NV, v, D, k)) == rule(U, row, NV, v, D, k)
    # [tile][S*E][D/8][clip][8]: clip 3's elements 24, 31 of slice 1 of tile 2 (NV = 4, D = 1024) -- unit 3 of the slice, 8 halves wide
    assert int(_run(driver, 8, 2 * 16 + 3, 4, 1, 1024, 24)) == ((2 * 4 + 1) * 128 + 3) * 128 + 3 * 8 + 0
    assert int(_run(driver, 8, 2 * 16 + 3, 4, 1, 1024, 31)) == ((2 * 4 + 1) * 128 + 3) * 128 + 3 * 8 + 7


# ---------------------------------------------------------------------------------------------------------------------------------
# the premise of the rank comparisons of tests/test_tiled16_gpu.py, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS + ["cfg1_10k"])
def test_rounded_goldens_keep_their_ranks_apart(name):
    """The oracle on the features rounded to binary16: neighbours in rank are more than 2e-12 apart on a prefix that keeps at least
    99 % of the ranks (so the cut of the GPU test drops at most 1 %), and cfg1_10k has no score within 2e-12 of its select's edges."""
    if name == "cfg1_10k":
        x16, t = cfg1_case16()
        present = None
    else:
        x16, _ids, present, t = golden_case16(name)
    sc = oracle_scores16(x16, t, present)
    k = rank_prefix(sc)
    print("%s as float16: %d of %d ranks settled" % (name, k, sc.size))
    assert k >= MIN_KEPT * sc.size, (k, sc.size)
    if name == "cfg1_10k":
        # 1e-12 of room for what the device's scores may differ from the oracle's by
        assert min(np.abs(sc - CFG1_BAND[0]).min(), np.abs(sc - CFG1_BAND[1]).min()) > GAP + 1e-12
        assert (sc >= CFG1_BAND[0]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# ShardedFeatureDB.set_layout over gloo
# ---------------------------------------------------------------------------------------------------------------------------------
def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _layout_worker(rank, world, port, tmp):
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from _standin_db import OracleFeatureDB
    from video_query_algorithms_amd import sharded_db
    from video_query_algorithms_amd.shard import shard_range

    class LayoutLog(OracleFeatureDB):                                  # the numpy stand-in, remembering every layout it was given
        def set_layout(self, layout):
            self.__dict__.setdefault("layouts", []).append(layout)
            OracleFeatureDB.set_layout(self, layout)
    n = 40
    x = np.random.default_rng(0).random((n, 2, 2, 8))
    r0, cnt = shard_range(n, world, rank)
    sdb = sharded_db.ShardedFeatureDB(LayoutLog(x[r0:r0 + cnt]), n, r0, np.arange(1, n + 1), served=True)
    order = ["tiled16", "rows", "tiled", "tiled64", "tiled16"]
    try:
        if rank == 0:
            sent = []
            real = type(sdb)._announce

            def recording(self, op, ints=(), floats=()):
                sent.append((op, [int(v) for v in ints]))
                return real(self, op, ints, floats)
            type(sdb)._announce = recording
            try:
                for name in order:
                    sdb.set_layout(name)
                with pytest.raises(KeyError):
                    sdb.set_layout("tiled128")                         # refused before anything is announced
            finally:
                type(sdb)._announce = real
            assert sent == [(sharded_db.OP_LAYOUT, [v]) for v in (3, 0, 1, 2, 3)], sent
            sdb.close()
        else:
            sdb.serve()
        assert sdb.local.layouts == order and sdb.local.layout == "tiled16", sdb.local.__dict__.get("layouts")
        open(os.path.join(tmp, "ok_%d" % rank), "w").close()
    finally:
        dist.destroy_process_group()


def test_sharded_set_layout_carries_tiled16_to_every_rank(tmp_path):
    import torch.multiprocessing as mp
    world = 3
    mp.spawn(_layout_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok_%d" % r)) for r in range(world))
