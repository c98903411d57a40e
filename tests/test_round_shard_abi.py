"""CPU: the entry points of include/vq_amd_round_shard.h (the avg rows of a batched round, and a group's whole weight update on avg tables
that come with the block: what a row-sharded database makes one operation of the update with) are declared, exported and bound,
their layouts are aligned, and every refusal that needs no round on a device returns its code -- the coverage
tests/test_round_update_abi.py gives include/vq_amd_round_update.h (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_round_shard.h"
NAMES = ["vq_db_batch_avg_rows_layout", "vq_db_batch_round_avg_rows", "vq_db_batch_round_update_given", "vq_db_batch_update_given_layout"]
# what earlier round headers declare and define: unchanged by this one
EARLIER = {"vq_amd_rounds.h": 4, "vq_amd_round_views.h": 3, "vq_amd_round_fit.h": 3, "vq_amd_round_targets.h": 2, "vq_amd_round_topk.h": 2,
           "vq_amd_round_grid.h": 2, "vq_amd_round_update.h": 2}


def _text(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return f.read()


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", _text(header), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def _handle():
    """A zeroed stand-in handle: the refusals under test come before the handle's state is read, and its S reads as 0."""
    return (ctypes.c_char * (1 << 16))()


def test_round_shard_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    assert _declared(HEADER) == NAMES == sorted(vqa._lib.ROUND_SHARD_SIGNATURES)
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    text = _text(HEADER)
    for name in NAMES:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.ROUND_SHARD_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.ROUND_SHARD_SIGNATURES[name]), name
    # every declaration cites the reference lines it restates
    cited = list(re.finditer(r"/\*((?:(?!\*/).)*)\*/\s*int\s+vq_", text, flags=re.S))
    assert len(cited) == len(NAMES)
    for decl in cited:
        assert re.search(r"(?:ticket|hyperparameter|compute_matches)\.py:\d+", decl.group(1)), decl.group(1)
    # additive: ABI 12 itself and the round headers before this one are untouched
    assert not set(NAMES) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols()) and not set(NAMES) & set(vqa._lib.exported_symbols())
    for header, count in EARLIER.items():
        assert len(_declared(header)) == count, header
    assert len(vqa._lib.ROUND_UPDATE_SIGNATURES) == 2 and len(vqa._lib.ROUND_GRID_SIGNATURES) == 2 and len(vqa._lib.ROUND_FIT_SIGNATURES) == 3
    # no new constant: the flags are those of the headers before
    assert re.findall(r"#define[ \t]+(\w+)", text) == ["VQ_AMD_ROUND_SHARD_H"]          # the include guard alone
    assert dict(re.findall(r"#define\s+(VQ_BUPDATE_\w+)\s+(\d+)", _text("vq_amd_round_update.h"))) == {"VQ_BUPDATE_SURFACE": "16",
                                                                                                         "VQ_BUPDATE_GIVEN_SURFACE": "32"}
    assert dict(re.findall(r"#define\s+(VQ_BROUND_\w+)\s+(\d+)", _text("vq_amd_rounds.h"))) == {"VQ_BROUND_AVG": "1", "VQ_BROUND_SCORES": "2",
                                                                                                 "VQ_BROUND_SELECT": "4", "VQ_BROUND_TIMED": "8"}
    # the code lives beside the calls it shares kernels with, each of the shared loops stated once, and reads no environment
    with open(os.path.join(ROOT, "video-query-algorithms_amd", "csrc", "vq_rounds.hip")) as f:
        unit = f.read()
    assert all(re.search(r"^int %s\(" % name, unit, flags=re.M) for name in NAMES) and "getenv" not in unit
    assert len(re.findall(r"__global__[^\n]*\bloss_surface_batch_kernel\(", unit)) == 1 and unit.count("ls_scores[l] = score_from_avg(") == 1
    assert len(re.findall(r"__global__[^\n]*\breview_band_batch_kernel\(", unit)) == 1 and len(re.findall(r"__global__[^\n]*\bavg_rows_batch_kernel\(", unit)) == 1


def test_the_main_header_brings_the_round_shard_calls_along_in_plain_c():
    assert '#include "%s"' % HEADER in _text("vq_amd.h")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int (*a)(vq_db*, int32_t, int64_t, int64_t*) = vq_db_batch_avg_rows_layout;\n'
                    ' int (*b)(vq_db*, int32_t, int64_t, void*, int64_t) = vq_db_batch_round_avg_rows;\n'
                    ' int (*f)(vq_db*, int32_t, int32_t, int32_t, int64_t, int64_t, int64_t*) = vq_db_batch_update_given_layout;\n'
                    ' int (*g)(vq_db*, int32_t, int32_t, int32_t, int64_t, int64_t, void*, int64_t, void*, int64_t, int32_t) = vq_db_batch_round_update_given;\n'
                    ' (void)a; (void)b; (void)f; (void)g; return VQ_BROUND_SCORES | VQ_BROUND_SELECT | VQ_BUPDATE_SURFACE; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_the_layouts_are_aligned_monotone_and_size_their_row_pieces_by_the_streams():
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    buf = _handle()
    S = 0                                                     # the streams of the zeroed handle (tests/test_batch_update_given_gpu.py: S = 2)
    off, plain, rows = (ctypes.c_int64 * 16)(), (ctypes.c_int64 * 16)(), (ctypes.c_int64 * 4)()
    for q, g, t, nl, nu in ((16, 64, 64, 4097, 333), (1, 1, 1, 0, 0), (3, 40, 31, 7, 0)):
        assert lib.vq_db_batch_update_given_layout(buf, q, g, t, nl, nu, off) == 0
        assert lib.vq_db_batch_update_layout(buf, q, g, t, nl, nu, plain) == 0
        o, p = list(off), list(plain)
        assert all(v % 64 == 0 for v in o) and o[0] == 0 and o == sorted(o) and o[:5] == p[:5]
        sizes = [q * g * 64, q * t * 8, q * 8, q * 8, nl * S * 8, nl * 8, q * g * t * 8, q * 4, q * 8, q * 4, q * 8, q * 8, nu * S * 8, q * 64, q * 16]
        assert all(o[i + 1] - o[i] >= size for i, size in enumerate(sizes)), (o, sizes)
        # every piece but the two row pieces has the size it has in the block of vq_db_batch_update_layout
        assert all(o[i + 1] - o[i] == p[i + 1] - p[i] for i in range(15) if i not in (4, 12))
        assert o[5] - o[4] == (nl * S * 8 + 63) // 64 * 64 and o[13] - o[12] == (nu * S * 8 + 63) // 64 * 64
        assert lib.vq_db_batch_avg_rows_layout(buf, q, nl, rows) == 0
        r = list(rows)
        assert all(v % 64 == 0 for v in r) and r[0] == 0 and r == sorted(r)
        assert r[1] - r[0] >= q * 8 and r[2] - r[1] >= nl * 8 and r[3] - r[2] == (nl * S * 8 + 63) // 64 * 64


def test_calls_on_a_null_handle_or_with_bad_arguments_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 16)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_update_given_layout", None, 4, 40, 31, 20, 0, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_avg_rows_layout", None, 4, 20, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = _handle()
    assert lib.vq_db_batch_update_given_layout(buf, 4, 40, 31, 20, 0, None) == -1
    assert lib.vq_db_batch_avg_rows_layout(buf, 4, 20, None) == -1
    # the shape checks come before the handle's state is read
    for q, g, t, nl, nu in ((0, 40, 31, 1, 0), (17, 40, 31, 1, 0), (4, 65, 31, 1, 0), (4, 0, 31, 1, 0), (4, 40, 65, 1, 0), (4, 40, 0, 1, 0),
                            (4, 40, 31, -1, 0), (4, 40, 31, 1, -1)):
        assert lib.vq_db_batch_update_given_layout(buf, q, g, t, nl, nu, off) == -1, (q, g, t, nl, nu)
        assert lib.vq_db_batch_round_update_given(buf, q, g, t, nl, nu, buf, 1 << 30, buf, 1 << 30, 6) == -1, (q, g, t, nl, nu)
    for q, n in ((0, 5), (17, 5), (4, -1), (4, (1 << 32) + 1)):
        assert lib.vq_db_batch_avg_rows_layout(buf, q, n, off) == -1, (q, n)
        assert lib.vq_db_batch_round_avg_rows(buf, q, n, buf, 1 << 30) == -1, (q, n)
    assert lib.vq_db_batch_update_given_layout(buf, 4, 40, 31, 20, 3, off) == 0
    need = off[15]
    big = (ctypes.c_char * need)()
    assert lib.vq_db_batch_round_update_given(None, 4, 40, 31, 20, 3, big, need, buf, 64, 6) == -1            # NULL handle
    assert lib.vq_db_batch_round_update_given(buf, 4, 40, 31, 20, 3, None, need, buf, 64, 6) == -1            # NULL update block
    assert lib.vq_db_batch_round_update_given(buf, 4, 40, 31, 20, 3, big, need, None, 0, 2) == -1             # scores back into no block
    assert lib.vq_db_batch_round_update_given(buf, 4, 40, 31, 20, 3, big, need, None, 0, 4) == -1             # lists back into no block
    for flags in (1, 8, 64, 6 | 128, -1, 32, 6 | 32, 16 | 32):                                                # unknown bits; a given surface
        assert lib.vq_db_batch_round_update_given(buf, 4, 40, 31, 20, 3, big, need, buf, 64, flags) == -1, flags
    assert "flags" in (lib.vq_last_error() or b"").decode()
    assert lib.vq_db_batch_round_update_given(buf, 4, 40, 31, 20, 3, big, need - 64, buf, 64, 6) == -1        # a short update block
    assert "vq_db_batch_update_given_layout" in (lib.vq_last_error() or b"").decode()
    rows = (ctypes.c_int64 * 4)()
    assert lib.vq_db_batch_avg_rows_layout(buf, 4, 20, rows) == 0
    small = (ctypes.c_char * rows[3])()
    assert lib.vq_db_batch_round_avg_rows(None, 4, 20, small, rows[3]) == -1                                  # NULL handle
    assert lib.vq_db_batch_round_avg_rows(buf, 4, 20, None, rows[3]) == -1                                    # NULL block
    assert lib.vq_db_batch_round_avg_rows(buf, 4, 20, small, rows[3] - 64) == -1                              # a short block
    assert "vq_db_batch_avg_rows_layout" in (lib.vq_last_error() or b"").decode()
    # behind the shape checks a handle without a batched round is VQ_E_STATE for both calls
    assert lib.vq_db_batch_round_avg_rows(buf, 4, 20, small, rows[3]) == -4
    assert lib.vq_db_batch_round_update_given(buf, 4, 40, 31, 20, 3, big, need, buf, 64, 6) == -4
