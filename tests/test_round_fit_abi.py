"""CPU: the entry points of include/vq_amd_round_fit.h (the weight fit and the re-weighting of a batched round's queries) are declared,
exported and bound -- the coverage tests/test_view_round_abi.py gives include/vq_amd_round_views.h, for the next header that is additive
to ABI 12 (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_round_fit.h"


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_round_fit_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared(HEADER)
    assert names == ["vq_db_batch_fit_layout", "vq_db_batch_round_fit", "vq_db_batch_round_rescore"]
    assert sorted(vqa._lib.ROUND_FIT_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        text = f.read()
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROUND_FIT_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROUND_FIT_SIGNATURES[name]), name
    # every declaration cites the reference lines it restates
    for decl in re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*int\s+vq_", text, flags=re.S):
        assert re.search(r"(?:ticket|hyperparameter|compute_matches)\.py:\d+", decl.group(1)), decl.group(1)
    # additive: ABI 12 itself and the three headers before this one are untouched
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols())
    assert not set(names) & set(vqa._lib.exported_symbols())
    assert len(_declared("vq_amd_rounds.h")) == 4 == len(vqa._lib.BATCH_ROUND_SIGNATURES)
    assert len(_declared("vq_amd_round_views.h")) == 3 == len(vqa._lib.VIEW_ROUND_SIGNATURES)
    assert len(_declared("vq_amd_rows.h")) == 4 == len(vqa._lib.ROW_VIEW_SIGNATURES)
    assert not re.search(r"#define\s+VQ_", re.sub(r"#define VQ_AMD_ROUND_FIT_H", "", text))        # the flags are the VQ_BROUND_* values


def test_the_main_header_brings_the_round_fit_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "%s"' % HEADER in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int (*f)(vq_db*, int32_t, int32_t, int32_t, int64_t, int64_t*) = vq_db_batch_fit_layout;\n'
                    ' int (*g)(vq_db*, int32_t, int32_t, int32_t, int64_t, void*, int64_t) = vq_db_batch_round_fit;\n'
                    ' int (*h)(vq_db*, int32_t, void*, int64_t, int32_t) = vq_db_batch_round_rescore; (void)f; (void)g; (void)h;\n'
                    ' return VQ_BROUND_SCORES | VQ_BROUND_SELECT; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_calls_on_a_null_handle_or_with_bad_shapes_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 8)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_fit_layout", None, 4, 40, 31, 20, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()
    assert lib.vq_db_batch_round_fit(None, 4, 40, 31, 20, buf, 64) == -1
    assert lib.vq_db_batch_round_rescore(None, 1, buf, 64, 6) == -1
    # the shape checks come before the handle is touched: any non-NULL pointer will do
    for q, g, t, nl in ((0, 40, 31, 1), (17, 40, 31, 1), (4, 65, 31, 1), (4, 0, 31, 1), (4, 40, 65, 1), (4, 40, 31, -1)):
        assert lib.vq_db_batch_fit_layout(buf, q, g, t, nl, off) == -1, (q, g, t, nl)
    assert lib.vq_db_batch_fit_layout(buf, 16, 64, 64, 4097, off) == 0
    o = list(off)
    assert all(v % 64 == 0 for v in o) and o[0] == 0 and o == sorted(o)
    assert o[1] - o[0] >= 16 * 64 * 64 and o[5] - o[4] >= 4097 * 8 and o[6] - o[5] >= 4097 * 8 and o[7] - o[6] >= 16 * 64 * 64 * 8
