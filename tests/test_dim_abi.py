"""CPU: include/vq_amd_dim.h (a logical vector length d on rows stored at a zero-padded pitch D, and the short-row scan kernel) is
additive to ABI 12 WITHOUT a new entry point: two flag bits in vq_db_create's dtype argument.  The header declares no function, the
library exports what it exported, the flags are bound, and every refusal that needs no device returns its code (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "vq_amd_dim.h"


def _text(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return f.read()


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", _text(header), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_dim_header_adds_two_flags_and_no_entry_point():
    import video_query_algorithms_amd as vqa
    text = _text(HEADER)
    assert _declared(HEADER) == []
    assert re.findall(r"#define[ \t]+(\w+)", text) == ["VQ_AMD_DIM_H", "VQ_DIM_PADDED", "VQ_DIM_SHORT_ROWS"]
    assert re.search(r"#define\s+VQ_DIM_PADDED\s+256\b", text) and re.search(r"#define\s+VQ_DIM_SHORT_ROWS\s+512\b", text)
    assert (vqa._lib.VQ_DIM_PADDED, vqa._lib.VQ_DIM_SHORT_ROWS) == (256, 512)
    # the bits lie above every storage type, and the header says what each entry point speaks on such a handle
    assert max(vqa._lib.VQ_F32, vqa._lib.VQ_F64, vqa._lib.VQ_F16) < 256
    assert "ticket.py:151" in text and "KEEPS SPEAKING THE STORED PITCH" in text and "UNPADDED rows" in text
    lib = vqa.load_library()
    assert lib.vq_abi_version() == 12 == vqa._lib.ABI_VERSION
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols())
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    for name in ("vq_db_create_dim", "vq_db_dim", "vq_db_upload_dim", "vq_db_scan_short"):
        assert not hasattr(raw, name), name
    # the switch is read by the scans' unit and listed with the others in the main header
    unit = open(os.path.join(ROOT, "video-query-algorithms_amd", "csrc", "vq_sim.hip")).read()
    assert 'getenv("VQ_SCAN_SHORT")' in unit and "VQ_SCAN_SHORT=0|1" in _text("vq_amd.h")
    assert len(re.findall(r"__global__[^\n]*\bscan_short_kernel\(", unit)) == 1
    db_unit = open(os.path.join(ROOT, "video-query-algorithms_amd", "csrc", "vq_db.hip")).read()
    assert len(re.findall(r"__global__[^\n]*\bpad_rows_kernel\(", db_unit)) == 1


def test_the_main_header_brings_the_flags_along_in_plain_c():
    assert '#include "%s"' % HEADER in _text("vq_amd.h")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\n'
                    'int main(void){ int32_t dtype = VQ_F64 | VQ_DIM_PADDED | VQ_DIM_SHORT_ROWS; return dtype == 769 ? VQ_OK : 1; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_creation_with_bad_arguments_fails_cleanly():
    import video_query_algorithms_amd as vqa
    lib = vqa.load_library()
    h = ctypes.c_void_p()
    P, SH = vqa._lib.VQ_DIM_PADDED, vqa._lib.VQ_DIM_SHORT_ROWS

    def last():
        return (lib.vq_last_error() or b"").decode()
    assert lib.vq_db_create(8, 2, 3, 101, P, 0, None) == -1 and "NULL" in last()
    # the shape checks come before any device call, with the flags as without
    for n, s, e, d, dtype in ((0, 2, 3, 101, P), (8, 0, 3, 101, P), (8, 2, 0, 101, P), (8, 2, 3, 0, P), (8, 2, 3, -5, P | SH), (8, 9, 1, 101, P),
                              (8, 8, 9, 101, SH), (8, 2, 3, 101, 1024), (8, 2, 3, 101, P | 2048), (8, 2, 3, (1 << 30) + 1, P), (8, 2, 3, 101, -1)):
        assert lib.vq_db_create(n, s, e, d, dtype, 0, ctypes.byref(h)) == -1, (n, s, e, d, dtype)
        assert not h.value
    assert lib.vq_db_create(8, 2, 3, 101, 1024, 0, ctypes.byref(h)) == -1 and "flag" in last()
    assert lib.vq_db_create(8, 2, 3, 101, P | 7, 0, ctypes.byref(h)) == -1 and "dtype" in last()
    # without the flags a length that is no multiple of 4 stays refused, with the message of ever
    for d in (1, 101, 1022, 1023):
        assert lib.vq_db_create(8, 2, 3, d, 0, 0, ctypes.byref(h)) == -1 and "multiple of 4" in last(), d


def test_the_host_class_pads_and_slices_without_a_device():
    """FeatureDB's own arithmetic on the two lengths, on an object made without a handle."""
    import numpy as np
    from video_query_algorithms_amd import feature_db
    for dim, pitch in ((1, 4), (3, 4), (4, 4), (101, 104), (127, 128), (129, 132), (1021, 1024), (1023, 1024), (1024, 1024)):
        db = feature_db.FeatureDB.__new__(feature_db.FeatureDB)
        db._h = None                                                          # nothing to close
        db.S, db.E, db.D, db.Dp, db.dtype = 2, 3, dim, (dim + 3) // 4 * 4, np.dtype(np.float32)
        assert db.Dp == pitch
        t = np.random.default_rng(dim).standard_normal((2, 3, dim))
        p = db._padded(t)
        assert p.shape == (2, 3, pitch) and p.flags.c_contiguous and (p[..., :dim] == t).all() and not p[..., dim:].any()
        assert not np.signbit(p[..., dim:]).any()                             # +0.0
        back = db._logical(p)
        assert back.shape == t.shape and back.flags.c_contiguous and (back == t).all()
        assert (p is t) == (dim == pitch)
        want = ("rows", "tiled") if pitch == 1024 else ("rows",)
        assert db.layouts == want and db.tiled_layout == (want[1] if pitch == 1024 else None)
        assert feature_db._pad_for(dim) is (True if dim % 4 else None)


def test_synthetic_refuses_a_length_that_is_no_multiple_of_4():
    import pytest
    from video_query_algorithms_amd import feature_db
    for dim in (1, 101, 1023):
        with pytest.raises(ValueError):
            feature_db.FeatureDB.synthetic(8, 2, 3, dim)
