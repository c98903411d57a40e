"""CPU: what VQ_LAYOUT_TILED64 (the tiled layout of float64 databases) adds outside the kernels.

  * the value: include/vq_amd.h and _lib agree on 2; additive to ABI 12 -- no new exported name;
  * the element-address rule (csrc/vq_tile_index.h), stated once and parametrised by the unit: compiled into a stand-alone host program
    (tests/sanitize/tile_index_driver.cc) under AddressSanitizer + UndefinedBehaviorSanitizer -- nothing sanitised is loaded here;
  * ShardedFeatureDB.set_layout over gloo, every rank's database a numpy stand-in: "tiled64" reaches every rank, and the
    announcement carries the layout's value ("rows" and "tiled" keep 0 and 1).

The GPU half is tests/test_tiled64_gpu.py."""
import glob
import os
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

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
    assert re.search(r"enum\s*\{\s*VQ_LAYOUT_ROWS = 0,\s*VQ_LAYOUT_TILED = 1,\s*VQ_LAYOUT_TILED64 = 2\s*\}", header)
    assert (vqa._lib.VQ_LAYOUT_ROWS, vqa._lib.VQ_LAYOUT_TILED, vqa._lib.VQ_LAYOUT_TILED64) == (0, 1, 2)
    assert re.search(r"#define\s+VQ_ABI_VERSION\s+12\b", header) and vqa.load_library().vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    # no new entry point: the main header still declares 102, and what the library exports is what the headers declare
    assert len(_declared(os.path.join(ROOT, "include", "vq_amd.h"))) == 102 == len(vqa._lib.exported_symbols())
    declared = set().union(*(_declared(h) for h in glob.glob(os.path.join(ROOT, "include", "*.h"))))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", vqa._lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("vq_")}
        assert exported == declared
    assert len(declared) == 130 and not any("tiled" in n or "64" in n for n in declared)
    # the names FeatureDB and ShardedFeatureDB speak are the header's values
    from video_query_algorithms_amd import feature_db, sharded_db
    assert feature_db._LAYOUTS == {"rows": 0, "tiled": 1, "tiled64": 2} == sharded_db.LAYOUT_VALUES


def test_the_rule_is_stated_once():
    """csrc/vq_db.hip (scale_query_kernel) and csrc/vq_csv.hip take the rule from the header: no copy of the formula is left anywhere."""
    users = []
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        if fn != "vq_tile_index.h":
            assert not re.search(r"int64_t\s+(feat_index|elem_index|tiled_index)\s*\(", text), fn
            assert "(row & 15)" not in text and "(clip & 15) *" not in text, fn
        if re.search(r"\bfeat_index\(", text) and fn != "vq_tile_index.h":
            users.append(fn)
    assert users == ["vq_csv.hip", "vq_db.hip"]
    assert '#include "vq_tile_index.h"' in open(os.path.join(CSRC, "vq_db.h")).read()
    for fn in users:
        assert '#include "vq_db.h"' in open(os.path.join(CSRC, fn)).read()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tile_index") / "tile_index_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "tile_index_driver.cc"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0 and not any(tag in r.stdout for tag in FINDINGS), r.stdout[-4000:]
    return r.stdout


def test_the_address_rule_is_a_bijection_onto_the_tiles_under_asan_ubsan(driver):
    """Units 2 and 4, ragged n, the largest shape: one to one onto the whole tiles, every row inside its tile's own bytes, unit 4 the
    fp32 formula as it was written before the header (the driver's own checks), and a few elements against the rule restated here."""
    assert _run(driver).strip().endswith("tile_index: ok")

    def rule(U, row, NV, v, D, k):
        if U == 0:
            return (row * NV + v) * D + k
        return ((((row >> 4) * NV + v) * (D // U) + k // U) * 16 + (row & 15)) * U + k % U
    rng = np.random.default_rng(2)
    for U in (0, 2, 4):
        for _ in range(6):
            NV, D = int(rng.integers(1, 11)), 1024
            row, v, k = int(rng.integers(0, 3_000_000)), int(rng.integers(0, NV)), int(rng.integers(0, D))      # past 2^31 elements
            assert int(_run(driver, U, row, NV, v, D, k)) == rule(U, row, NV, v, D, k)
    # [tile][S*E][D/2][clip][2]: clip 3's elements 6, 7 of slice 1 of tile 2 (NV = 4, D = 1024) -- unit 3 of the slice, 2 doubles wide
    assert int(_run(driver, 2, 2 * 16 + 3, 4, 1, 1024, 6)) == ((2 * 4 + 1) * 512 + 3) * 32 + 3 * 2 + 0
    assert int(_run(driver, 2, 2 * 16 + 3, 4, 1, 1024, 7)) == ((2 * 4 + 1) * 512 + 3) * 32 + 3 * 2 + 1


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
    order = ["tiled64", "rows", "tiled"]
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
            assert sent == [(sharded_db.OP_LAYOUT, [2]), (sharded_db.OP_LAYOUT, [0]), (sharded_db.OP_LAYOUT, [1])], sent
            sdb.close()
        else:
            sdb.serve()
        assert sdb.local.layouts == order and sdb.local.layout == "tiled", sdb.local.__dict__.get("layouts")
        open(os.path.join(tmp, "ok_%d" % rank), "w").close()
    finally:
        dist.destroy_process_group()


def test_sharded_set_layout_reaches_every_rank_with_the_layouts_value(tmp_path):
    import torch.multiprocessing as mp
    world = 3
    mp.spawn(_layout_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok_%d" % r)) for r in range(world))
