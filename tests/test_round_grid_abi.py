"""CPU: the entry points of include/vq_amd_round_grid.h (the scores of chosen rows of a batched round under a grid of weights, for
every query in one call) are declared, exported and bound -- the coverage tests/test_round_topk_abi.py gives
include/vq_amd_round_topk.h, for the next header that is additive to ABI 12 (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_round_grid.h"
NAMES = ["vq_db_batch_grid_layout", "vq_db_batch_round_grid"]
MAX_GRID = 64                                  # the largest n_grid, as the header's text states it


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_round_grid_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared(HEADER)
    assert names == NAMES
    assert sorted(vqa._lib.ROUND_GRID_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        text = f.read()
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROUND_GRID_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROUND_GRID_SIGNATURES[name]), name
    # the two signatures as the issue fixes them
    assert re.search(r"int\s+vq_db_batch_grid_layout\(vq_db\* db, int32_t n_queries, int32_t n_grid, int64_t n_rows, int64_t\* off\);", text)
    assert re.search(r"int\s+vq_db_batch_round_grid\(vq_db\* db, int32_t n_queries, int32_t n_grid, int64_t n_rows, void\* block, "
                     r"int64_t block_bytes\);", text)
    # every declaration cites the reference line it restates
    cited = list(re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*int\s+vq_", text, flags=re.S))
    assert len(cited) == 2
    for decl in cited:
        assert re.search(r"hyperparameter\.py:57-58", decl.group(1)), decl.group(1)
    # the scope limits are stated in the header's text
    for phrase in ("OUT OF SCOPE", "query_round_batch_sets", "vq_db_batch_targets", "minimum", "second GPU"):
        assert phrase in text, phrase
    # additive: ABI 12 itself and the headers before this one are untouched
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols())
    assert not set(names) & set(vqa._lib.exported_symbols())
    earlier = {"vq_amd_rows.h": vqa._lib.ROW_VIEW_SIGNATURES, "vq_amd_rounds.h": vqa._lib.BATCH_ROUND_SIGNATURES,
               "vq_amd_round_views.h": vqa._lib.VIEW_ROUND_SIGNATURES, "vq_amd_round_fit.h": vqa._lib.ROUND_FIT_SIGNATURES,
               "vq_amd_round_targets.h": vqa._lib.ROUND_TARGETS_SIGNATURES, "vq_amd_round_topk.h": vqa._lib.ROUND_TOPK_SIGNATURES}
    for header, count in zip(earlier, (4, 4, 3, 3, 2, 2)):
        assert len(_declared(header)) == count == len(earlier[header]), header
        assert not set(names) & set(_declared(header)), header
    assert (vqa._lib.VQ_BROUND_AVG, vqa._lib.VQ_BROUND_SCORES, vqa._lib.VQ_BROUND_SELECT, vqa._lib.VQ_BROUND_TIMED) == (1, 2, 4, 8)
    assert not re.search(r"#define\s+VQ_", re.sub(r"#define VQ_AMD_ROUND_GRID_H", "", text))      # no new constant, no switch
    unit = open(os.path.join(ROOT, "video-query-algorithms_amd", "csrc", "vq_rounds.hip")).read()
    assert "getenv" not in unit and re.search(r"__global__[^\n]*\bgrid_scores_batch_kernel\(", unit)


def test_the_main_header_brings_the_round_grid_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "%s"' % HEADER in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int (*f)(vq_db*, int32_t, int32_t, int64_t, int64_t*) = vq_db_batch_grid_layout;\n'
                    ' int (*g)(vq_db*, int32_t, int32_t, int64_t, void*, int64_t) = vq_db_batch_round_grid; (void)f; (void)g;\n'
                    ' return VQ_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_the_score_of_a_clip_keeps_its_one_definition():
    """The grid kernel scores with the function the scans, the fit and the rescore use: its bits are theirs by construction."""
    csrc = os.path.join(ROOT, "video-query-algorithms_amd", "csrc")
    found = [fn for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h")) and re.search(r"double\s+score_from_avg\s*\(", open(os.path.join(csrc, fn)).read())]
    assert found == ["vq_score.h"]
    unit = open(os.path.join(csrc, "vq_rounds.hip")).read()
    body = unit[unit.index("void grid_scores_batch_kernel("):]
    assert "score_from_avg(" in body[:body.index("\n}\n")]


def test_calls_on_a_null_handle_or_with_bad_shapes_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 5)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_grid_layout", None, 4, 40, 20, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()
    assert lib.vq_db_batch_round_grid(None, 4, 40, 20, buf, 64) == -1
    assert lib.vq_db_batch_round_grid(buf, 4, 40, 20, None, 64) == -1
    assert lib.vq_db_batch_grid_layout(buf, 4, 40, 20, None) == -1
    # the shape checks come before the handle is touched: any non-NULL pointer will do
    for q, g, n in ((0, 40, 20), (17, 40, 20), (-1, 40, 20), (4, 0, 20), (4, -1, 20), (4, MAX_GRID + 1, 20), (4, 40, -1)):
        assert lib.vq_db_batch_grid_layout(buf, q, g, n, off) == -1, (q, g, n)
        assert lib.vq_db_batch_round_grid(buf, q, g, n, buf, 64) == -1, (q, g, n)
    # so does the size of the block: a short one is refused before the handle's lock is taken
    assert lib.vq_db_batch_round_grid(buf, 4, 40, 20, buf, 64) == -1


def test_layouts_are_ordered_aligned_and_roomy():
    """Q = 16, G = 64, and the smallest call.  There is no device here, so the handle is a zeroed stand-in: the layout depends on the
    arguments only."""
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    handle = (ctypes.c_char * 65536)()
    off = (ctypes.c_int64 * 5)()
    for q, g, n in ((16, MAX_GRID, 16 * 300), (1, 1, 1), (3, 40, 21), (2, 5, 0)):
        assert lib.vq_db_batch_grid_layout(handle, q, g, n, off) == 0
        o = list(off)
        assert all(v % 64 == 0 for v in o) and o[0] == 0 and o == sorted(o)
        room = [o[i + 1] - o[i] for i in range(4)]
        assert room[0] >= q * g * 8 * 8 and room[1] >= q * 8 and room[2] >= n * 8 and room[3] >= g * n * 8
