"""CPU: the batched-round entry points (include/vq_amd_rounds.h) are declared, exported and bound -- the coverage tests/test_abi.py
gives include/vq_amd.h, for the header that is additive to ABI 12 (no compute calls)."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_batch_round_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared("vq_amd_rounds.h")
    assert names == ["vq_db_batch_round_fetch", "vq_db_batch_round_layout", "vq_db_batch_round_times", "vq_db_query_round_batch"]
    assert sorted(vqa._lib.BATCH_ROUND_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "vq_amd_rounds.h")) as f:
        text = f.read()
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.BATCH_ROUND_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(vqa._lib.BATCH_ROUND_SIGNATURES[name]), name
    # additive: ABI 12 itself is untouched
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12
    assert len(_declared("vq_amd.h")) == 102 == len(vqa._lib.exported_symbols())
    assert not set(names) & set(vqa._lib.exported_symbols())
    flags = dict(re.findall(r"#define (VQ_BROUND_\w+) (\d+)", text))
    assert {k: int(v) for k, v in flags.items()} == {"VQ_BROUND_AVG": vqa._lib.VQ_BROUND_AVG, "VQ_BROUND_SCORES": vqa._lib.VQ_BROUND_SCORES,
                                                     "VQ_BROUND_SELECT": vqa._lib.VQ_BROUND_SELECT, "VQ_BROUND_TIMED": vqa._lib.VQ_BROUND_TIMED}


def test_the_main_header_brings_the_batched_rounds_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "vq_amd_rounds.h"' in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\nint main(void){ int (*f)(vq_db*, int32_t, void*, int64_t, int32_t) = vq_db_query_round_batch; (void)f; '
                    'return VQ_BROUND_AVG | VQ_BROUND_SELECT; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_calls_on_a_null_handle_fail_cleanly():
    import pytest
    import video_query_algorithms_amd as vqa
    off = (ctypes.c_int64 * 12)()
    with pytest.raises(vqa.VqError) as ei:
        vqa._lib.call("vq_db_batch_round_layout", None, 4, off)
    assert ei.value.code == -1 and "NULL" in str(ei.value)
    lib = vqa.load_library()
    buf = (ctypes.c_char * 64)()
    assert lib.vq_db_query_round_batch(None, 4, buf, 64, 7) == -1
    assert lib.vq_db_batch_round_fetch(None, 0, None, 0, None, 0) == -1
    assert lib.vq_db_batch_round_times(None, (ctypes.c_float * 3)()) == -1
