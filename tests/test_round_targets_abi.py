"""CPU: the entry points of include/vq_amd_round_targets.h (the bootstrapped targets of a group of tickets in one call) are declared,
exported and bound -- the coverage tests/test_round_fit_abi.py gives include/vq_amd_round_fit.h, for the next header that is additive
to ABI 12 (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_round_targets.h"
NAMES = ["vq_db_batch_targets", "vq_db_batch_targets_layout"]


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_round_targets_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared(HEADER)
    assert names == NAMES
    assert sorted(vqa._lib.ROUND_TARGETS_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        text = f.read()
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROUND_TARGETS_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROUND_TARGETS_SIGNATURES[name]), name
    # the two signatures as the issue fixes them
    assert re.search(r"int\s+vq_db_batch_targets_layout\(vq_db\* db, int32_t n_queries, int64_t n_pool_rows, int32_t n_draws, int64_t n_entries, "
                     r"int64_t\* off\);", text)
    assert re.search(r"int\s+vq_db_batch_targets\(vq_db\* db, int32_t n_queries, int64_t n_pool_rows, int32_t n_draws, int64_t n_entries, void\* block, "
                     r"int64_t block_bytes\);", text)
    # every declaration cites the reference lines it restates
    cited = list(re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*int\s+vq_", text, flags=re.S))
    assert len(cited) == 2
    for decl in cited:
        assert re.search(r"target_clip\.py:\d+", decl.group(1)), decl.group(1)
    # additive: ABI 12 itself and the headers before this one are untouched
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols())
    assert not set(names) & set(vqa._lib.exported_symbols())
    assert len(_declared("vq_amd_rows.h")) == 4 == len(vqa._lib.ROW_VIEW_SIGNATURES)
    assert len(_declared("vq_amd_rounds.h")) == 4 == len(vqa._lib.BATCH_ROUND_SIGNATURES)
    assert len(_declared("vq_amd_round_views.h")) == 3 == len(vqa._lib.VIEW_ROUND_SIGNATURES)
    assert len(_declared("vq_amd_round_fit.h")) == 3 == len(vqa._lib.ROUND_FIT_SIGNATURES)
    assert not re.search(r"#define\s+VQ_", re.sub(r"#define VQ_AMD_ROUND_TARGETS_H", "", text))      # no new constant, no switch
    assert "getenv" not in open(os.path.join(ROOT, "video-query-algorithms_amd", "csrc", "vq_round_targets.hip")).read()


def test_the_main_header_brings_the_round_targets_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "%s"' % HEADER in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int (*f)(vq_db*, int32_t, int64_t, int32_t, int64_t, int64_t*) = vq_db_batch_targets_layout;\n'
                    ' int (*g)(vq_db*, int32_t, int64_t, int32_t, int64_t, void*, int64_t) = vq_db_batch_targets; (void)f; (void)g;\n'
                    ' return VQ_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_calls_on_a_null_handle_or_with_bad_shapes_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 11)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_targets_layout", None, 4, 80, 12, 150, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()
    assert lib.vq_db_batch_targets(None, 4, 80, 12, 150, buf, 64) == -1
    assert lib.vq_db_batch_targets(buf, 4, 80, 12, 150, None, 64) == -1
    assert lib.vq_db_batch_targets_layout(buf, 4, 80, 12, 150, None) == -1
    # the shape checks come before the handle is touched: any non-NULL pointer will do
    bad = ((0, 1, 1, 1), (17, 17, 17, 17), (4, 3, 12, 150), (4, 4 * 256 + 1, 12, 150), (4, 80, 3, 150), (4, 80, 4 * 64 + 1, 300),
           (4, 80, 12, 11), (4, 80, 12, 12 * 256 + 1), (4, -1, 12, 150), (4, 80, -1, 150), (4, 80, 12, -1))
    for q, nr, nd, ne in bad:
        assert lib.vq_db_batch_targets_layout(buf, q, nr, nd, ne, off) == -1, (q, nr, nd, ne)
        assert lib.vq_db_batch_targets(buf, q, nr, nd, ne, buf, 64) == -1, (q, nr, nd, ne)


def test_a_maximal_layout_is_ordered_aligned_and_roomy():
    """Q = 16, 256-row pools, 64 draws each, every draw the whole pool.  There is no device here, so the handle is a zeroed stand-in: its
    S, E, D read as 0, the two [Q][S][E][D] pieces come out empty, and every piece whose size the arguments fix is measured
    (tests/test_batch_targets_gpu.py measures those two on a real handle)."""
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    handle = (ctypes.c_char * 65536)()
    off = (ctypes.c_int64 * 11)()
    Q, rows, n_draws, entries = 16, 16 * 256, 16 * 64, 16 * 64 * 256
    assert lib.vq_db_batch_targets_layout(handle, Q, rows, n_draws, entries, off) == 0
    o = list(off)[:10]
    assert all(v % 64 == 0 for v in o) and o[0] == 0 and o == sorted(o)
    room = [o[i + 1] - o[i] for i in range(9)]
    assert room[0] >= Q * 8 * 4 and room[1] >= Q * 4 * 8 and room[2] >= rows * 8 and room[3] >= n_draws * 2 * 4 and room[4] >= entries * 4
    assert room[5] >= n_draws * 4 and room[7] >= Q * 4 * 4
    assert 1 <= off[10] <= 256
    # the smallest call
    assert lib.vq_db_batch_targets_layout(handle, 1, 1, 1, 1, off) == 0
    assert list(off)[:10] == sorted(list(off)[:10]) and all(v % 64 == 0 for v in list(off)[:10])
