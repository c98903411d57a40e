"""CPU: the entry points of include/vq_amd_round_topk.h (the k best clips of every query of a batched round in one call) are declared,
exported and bound -- the coverage tests/test_round_targets_abi.py gives include/vq_amd_round_targets.h, for the next header that is
additive to ABI 12 (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_round_topk.h"
NAMES = ["vq_db_batch_round_topk", "vq_db_batch_topk_layout"]
CAP = 4096                                     # the largest k_max, as the header's text states it


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_round_topk_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared(HEADER)
    assert names == NAMES
    assert sorted(vqa._lib.ROUND_TOPK_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        text = f.read()
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROUND_TOPK_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROUND_TOPK_SIGNATURES[name]), name
    # the two signatures as the issue fixes them
    assert re.search(r"int\s+vq_db_batch_topk_layout\(vq_db\* db, int32_t n_queries, int64_t k_max, int64_t\* off\);", text)
    assert re.search(r"int\s+vq_db_batch_round_topk\(vq_db\* db, int32_t n_queries, int64_t k_max, void\* block, int64_t block_bytes\);", text)
    # every declaration cites the reference line it restates
    cited = list(re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*int\s+vq_", text, flags=re.S))
    assert len(cited) == 2
    for decl in cited:
        assert re.search(r"ticket\.py:266", decl.group(1)), decl.group(1)
    # the cap is stated in the header's text
    assert re.search(r"off\[5\] = the largest k_max the call accepts: %d\b" % CAP, text)
    # additive: ABI 12 itself and the headers before this one are untouched
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols())
    assert not set(names) & set(vqa._lib.exported_symbols())
    earlier = {"vq_amd_rows.h": vqa._lib.ROW_VIEW_SIGNATURES, "vq_amd_rounds.h": vqa._lib.BATCH_ROUND_SIGNATURES,
               "vq_amd_round_views.h": vqa._lib.VIEW_ROUND_SIGNATURES, "vq_amd_round_fit.h": vqa._lib.ROUND_FIT_SIGNATURES,
               "vq_amd_round_targets.h": vqa._lib.ROUND_TARGETS_SIGNATURES}
    for header, count in zip(earlier, (4, 4, 3, 3, 2)):
        assert len(_declared(header)) == count == len(earlier[header]), header
        assert not set(names) & set(_declared(header)), header
    assert (vqa._lib.VQ_BROUND_AVG, vqa._lib.VQ_BROUND_SCORES, vqa._lib.VQ_BROUND_SELECT, vqa._lib.VQ_BROUND_TIMED) == (1, 2, 4, 8)
    assert not re.search(r"#define\s+VQ_", re.sub(r"#define VQ_AMD_ROUND_TOPK_H", "", text))      # no new constant, no switch
    assert "getenv" not in open(os.path.join(ROOT, "video-query-algorithms_amd", "csrc", "vq_round_topk.hip")).read()


def test_the_main_header_brings_the_round_topk_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "%s"' % HEADER in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int (*f)(vq_db*, int32_t, int64_t, int64_t*) = vq_db_batch_topk_layout;\n'
                    ' int (*g)(vq_db*, int32_t, int64_t, void*, int64_t) = vq_db_batch_round_topk; (void)f; (void)g;\n'
                    ' return VQ_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_order_key_has_one_definition():
    """The key of a ranking and the selection helpers live in one header that every unit using them includes (csrc/vq_db.hip takes the
    block size of the selection scratch from it)."""
    csrc = os.path.join(ROOT, "video-query-algorithms_amd", "csrc")
    found = [fn for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h")) and re.search(r"uint64_t\s+order_key\s*\(", open(os.path.join(csrc, fn)).read())]
    assert found == ["vq_select.h"]
    for unit in ("vq_rank.hip", "vq_db.hip", "vq_rounds.hip", "vq_round_topk.hip"):
        assert '#include "vq_select.h"' in open(os.path.join(csrc, unit)).read(), unit


def test_calls_on_a_null_handle_or_with_bad_shapes_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 6)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_topk_layout", None, 4, 20, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()
    assert lib.vq_db_batch_round_topk(None, 4, 20, buf, 64) == -1
    assert lib.vq_db_batch_round_topk(buf, 4, 20, None, 64) == -1
    assert lib.vq_db_batch_topk_layout(buf, 4, 20, None) == -1
    # the shape checks come before the handle is touched: any non-NULL pointer will do
    for q, k_max in ((0, 20), (17, 20), (-1, 20), (4, 0), (4, -1), (4, CAP + 1)):
        assert lib.vq_db_batch_topk_layout(buf, q, k_max, off) == -1, (q, k_max)
        assert lib.vq_db_batch_round_topk(buf, q, k_max, buf, 64) == -1, (q, k_max)


def test_a_maximal_layout_is_ordered_aligned_and_roomy():
    """Q = 16, k_max = the cap.  There is no device here, so the handle is a zeroed stand-in: the layout depends on the arguments only."""
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    handle = (ctypes.c_char * 65536)()
    off = (ctypes.c_int64 * 6)()
    Q = 16
    assert lib.vq_db_batch_topk_layout(handle, Q, CAP, off) == 0
    o = list(off)[:5]
    assert all(v % 64 == 0 for v in o) and o[0] == 0 and o == sorted(o)
    room = [o[i + 1] - o[i] for i in range(4)]
    assert room[0] >= Q * 8 and room[1] >= Q * 8 and room[2] >= Q * CAP * 8 and room[3] >= Q * CAP * 8
    assert off[5] == CAP
    # the smallest call, and an odd one
    for q, k_max in ((1, 1), (3, 21)):
        assert lib.vq_db_batch_topk_layout(handle, q, k_max, off) == 0
        o = list(off)[:5]
        assert o == sorted(o) and all(v % 64 == 0 for v in o) and off[5] == CAP
        assert o[1] - o[0] >= q * 8 and o[2] - o[1] >= q * 8 and o[3] - o[2] >= q * k_max * 8 and o[4] - o[3] >= q * k_max * 8
