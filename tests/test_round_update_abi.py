"""CPU: the entry points of include/vq_amd_round_update.h (a group's whole weight update on a batched round in one call) are declared,
exported and bound, their layout is aligned, and every refusal that needs no round on a device returns its code -- the coverage
tests/test_round_fit_abi.py gives include/vq_amd_round_fit.h (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_round_update.h"
NAMES = ["vq_db_batch_round_update", "vq_db_batch_update_layout"]


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_round_update_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    assert _declared(HEADER) == NAMES == sorted(vqa._lib.ROUND_UPDATE_SIGNATURES)
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", HEADER)) as f:
        text = f.read()
    for name in NAMES:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROUND_UPDATE_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROUND_UPDATE_SIGNATURES[name]), name
    # every declaration cites the reference lines it restates
    for decl in re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*int\s+vq_", text, flags=re.S):
        assert re.search(r"(?:ticket|hyperparameter|compute_matches)\.py:\d+", decl.group(1)), decl.group(1)
    # additive: ABI 12 itself and the round headers before this one are untouched
    assert not set(NAMES) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols()) and not set(NAMES) & set(vqa._lib.exported_symbols())
    assert len(_declared("vq_amd_round_fit.h")) == 3 == len(vqa._lib.ROUND_FIT_SIGNATURES)
    flags = dict(re.findall(r"#define\s+(VQ_BUPDATE_\w+)\s+(\d+)", text))
    assert flags == {"VQ_BUPDATE_SURFACE": str(vqa._lib.VQ_BUPDATE_SURFACE), "VQ_BUPDATE_GIVEN_SURFACE": str(vqa._lib.VQ_BUPDATE_GIVEN_SURFACE)}
    # the new bits do not collide with the VQ_BROUND_* ones they are combined with
    assert not (vqa._lib.VQ_BUPDATE_SURFACE | vqa._lib.VQ_BUPDATE_GIVEN_SURFACE) & 15


def test_the_main_header_brings_the_round_update_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "%s"' % HEADER in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int (*f)(vq_db*, int32_t, int32_t, int32_t, int64_t, int64_t, int64_t*) = vq_db_batch_update_layout;\n'
                    ' int (*g)(vq_db*, int32_t, int32_t, int32_t, int64_t, int64_t, void*, int64_t, void*, int64_t, int32_t) = vq_db_batch_round_update;\n'
                    ' (void)f; (void)g; return VQ_BROUND_SCORES | VQ_BROUND_SELECT | VQ_BUPDATE_SURFACE | VQ_BUPDATE_GIVEN_SURFACE; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_the_layout_is_aligned_monotone_and_starts_like_the_fit_block():
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()                              # the layout reads nothing of the handle: any non-NULL pointer will do
    off, fit = (ctypes.c_int64 * 16)(), (ctypes.c_int64 * 8)()
    for q, g, t, nl, nu in ((16, 64, 64, 4097, 333), (1, 1, 1, 0, 0), (3, 40, 31, 7, 0), (16, 40, 31, 960, 16 * 200)):
        assert lib.vq_db_batch_update_layout(buf, q, g, t, nl, nu, off) == 0
        assert lib.vq_db_batch_fit_layout(buf, q, g, t, nl, fit) == 0
        o = list(off)
        assert all(v % 64 == 0 for v in o) and o[0] == 0 and o == sorted(o) and o[:7] == list(fit)[:7]
        sizes = [q * g * 64, q * t * 8, q * 8, q * 8, nl * 8, nl * 8, q * g * t * 8, q * 4, q * 8, q * 4, q * 8, q * 8, nu * 8, q * 64, q * 16]
        assert all(o[i + 1] - o[i] >= size for i, size in enumerate(sizes)), (o, sizes)


def test_calls_on_a_null_handle_or_with_bad_arguments_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 16)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_update_layout", None, 4, 40, 31, 20, 0, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()
    assert lib.vq_db_batch_update_layout(buf, 4, 40, 31, 20, 0, None) == -1
    # the shape checks come before the handle is touched: any non-NULL pointer will do
    for q, g, t, nl, nu in ((0, 40, 31, 1, 0), (17, 40, 31, 1, 0), (4, 65, 31, 1, 0), (4, 0, 31, 1, 0), (4, 40, 65, 1, 0), (4, 40, 0, 1, 0),
                            (4, 40, 31, -1, 0), (4, 40, 31, 1, -1)):
        assert lib.vq_db_batch_update_layout(buf, q, g, t, nl, nu, off) == -1, (q, g, t, nl, nu)
        assert lib.vq_db_batch_round_update(buf, q, g, t, nl, nu, buf, 1 << 30, buf, 1 << 30, 6) == -1, (q, g, t, nl, nu)
    assert lib.vq_db_batch_update_layout(buf, 4, 40, 31, 20, 3, off) == 0
    need = off[15]
    big = (ctypes.c_char * need)()
    assert lib.vq_db_batch_round_update(None, 4, 40, 31, 20, 3, big, need, buf, 64, 6) == -1                  # NULL handle
    assert lib.vq_db_batch_round_update(buf, 4, 40, 31, 20, 3, None, need, buf, 64, 6) == -1                  # NULL update block
    assert lib.vq_db_batch_round_update(buf, 4, 40, 31, 20, 3, big, need, None, 0, 2) == -1                   # scores back into no block
    assert lib.vq_db_batch_round_update(buf, 4, 40, 31, 20, 3, big, need, None, 0, 4) == -1                   # lists back into no block
    for flags in (1, 8, 64, 6 | 128, -1, 16 | 32):                                                            # unknown bits; both surface bits
        assert lib.vq_db_batch_round_update(buf, 4, 40, 31, 20, 3, big, need, buf, 64, flags) == -1, flags
    assert lib.vq_db_batch_round_update(buf, 4, 40, 31, 20, 3, big, need - 64, buf, 64, 6) == -1              # a short update block
    assert "vq_db_batch_update_layout" in (lib.vq_last_error() or b"").decode()
