"""CPU: the row-view entry points (include/vq_amd_rows.h) are declared, exported and bound -- the coverage tests/test_abi.py gives
include/vq_amd.h, for the header that is additive to ABI 12 (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_row_view_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared("vq_amd_rows.h")
    assert names == ["vq_db_rows_active", "vq_db_rows_define", "vq_db_rows_drop", "vq_db_rows_use"]
    assert sorted(vqa._lib.ROW_VIEW_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROW_VIEW_SIGNATURES[name]
    with open(os.path.join(ROOT, "include", "vq_amd_rows.h")) as f:
        text = f.read()
    for name in names:
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROW_VIEW_SIGNATURES[name]), name
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12      # additive: ABI 12 itself is untouched


def test_the_main_header_brings_the_row_views_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "vq_amd_rows.h"' in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\nint main(void){ int (*f)(vq_db*, const int64_t*, int64_t, int32_t*) = vq_db_rows_define; (void)f; return VQ_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])
