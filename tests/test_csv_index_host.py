"""CPU: the line index of a feature CSV file (vq_csv_index, csrc/host/vq_csv_read.cc) against the reference's reader
(tsn/feature_csv.read_features: csv.reader, int(row[0]), float(x)), through the stand-alone ASan + UBSan driver of tests/sanitize_csv;
and the two new entry points in the header, the library and the ctypes table (include/vq_amd_csv.h, additive to ABI 12)."""
import ctypes
import lzma
import glob
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _csv_driver as cd
from _helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"video =v, video url =/a/v.mp4, CNN stream =rgb, feature blob =global_pool, caffe model =m.caffemodel"


def _python(path):
    from video_query_algorithms_amd.tsn import feature_csv
    try:
        _meta, clips, feats = feature_csv.read_features(path)
    except Exception:
        return None
    if clips.size == 0:                                   # a header alone: no rows, no dim
        return clips, feats.reshape(0, 0)
    if feats.ndim != 2 or feats.shape[0] != clips.shape[0]:
        return None
    return clips, feats


def _parse_answers(text):
    """the driver's 'parse' output -> per file: None (refused, with the message) or (header_bytes, clips, bits [n, dim], host_fields)"""
    out = []
    blocks = re.split(r"^file \d+\n", text, flags=re.M)[1:]
    for b in blocks:
        lines = b.rstrip("\n").split("\n")
        if lines[0].startswith("error"):
            out.append((None, lines[0]))
            continue
        w = lines[0].split()
        assert w[0] == "ok", b[:200]
        n, dim = int(w[4]), int(w[6])
        clips = np.array([int(x) for x in (lines[1].split() if n else [])], dtype=np.int64)
        bits = np.array([[int(x, 16) for x in ln.split()] for ln in lines[2:2 + n]], dtype=np.uint64).reshape(n, dim)
        out.append(((int(w[2]), clips, bits, int(w[8])), lines[0]))
    return out


def _agrees(answer, py):
    hb, clips, bits, _host = answer
    return py is not None and (py[0] == clips).all() and py[1].shape == bits.shape and (np.ascontiguousarray(py[1]).view(np.uint64) == bits).all()


def _rows(rng, n, d, fmt="repr"):
    from video_query_algorithms_amd.tsn.feature_csv import NUMBER_FORMATS
    x = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-8, 8, (n, d))
    return "".join("%d,%s\n" % (i + 1, ",".join(NUMBER_FORMATS[fmt](v) for v in row)) for i, row in enumerate(x.tolist())).encode(), x


def test_the_shipped_files_with_lf_crlf_and_no_final_newline(tmp_path):
    paths = []
    for k, src in enumerate(sorted(glob.glob(os.path.join(GOLDEN, "reference_features", "**", "*.csv.xz"), recursive=True))[:3]):
        with lzma.open(src) as f:
            data = f.read()
        for name, body in (("lf", data), ("crlf", data.replace(b"\n", b"\r\n")), ("cut", data.rstrip(b"\n"))):
            paths.append(str(tmp_path / ("g%d_%s.csv" % (k, name))))
            with open(paths[-1], "wb") as g:
                g.write(body)
    answers = _parse_answers(cd.run("parse", *paths))
    assert len(answers) == len(paths)
    for path, (ans, line) in zip(paths, answers):
        assert ans is not None and _agrees(ans, _python(path)), (path, line)
        assert ans[3] == 0 and ans[2].shape[1] == 1024                                   # no field of the shipped files needs the host
        with open(path, "rb") as f:
            assert ans[0] == len(f.readline().rstrip(b"\r\n"))


def test_offsets_small_shapes_and_refusals(tmp_path):
    rng = np.random.default_rng(1)
    body, _x = _rows(rng, 3, 1)
    cases = {
        "d1": HEADER + b"\n" + body,                                                     # D = 1
        "d101": HEADER + b"\r\n" + _rows(rng, 4, 101, "g12")[0].replace(b"\n", b"\r\n"),
        "header_only": HEADER + b"\n",
        "header_cut": HEADER,
        "empty_line": HEADER + b"\n1,0.5\n\n2,0.25\n",
        "empty_line_crlf": HEADER + b"\r\n1,0.5\r\n\r\n",
        "short_row": HEADER + b"\n1,0.5,0.25\n2,0.5\n",
        "long_row": HEADER + b"\n1,0.5\n2,0.5,0.25\n",
        "quote": HEADER + b"\n1,\"0.5\"\n",
        "bare_cr": HEADER + b"\n1,0.5\r2,0.5\n",
        "no_value": HEADER + b"\n1\n",
        "clip_text": HEADER + b"\n1.0,0.5\n",
        "garbage_field": HEADER + b"\n1,0.5,2.5\n2,0.5,2.5x\n",
        "empty_file": b"",
        "blanks_and_words": HEADER + b"\n 7 , 1.5,\tinf ,-NaN\n+8,1e5,.5,5.\n",
    }
    paths = {}
    for name, data in cases.items():
        paths[name] = str(tmp_path / (name + ".csv"))
        with open(paths[name], "wb") as f:
            f.write(data)
    names = list(cases)
    answers = dict(zip(names, _parse_answers(cd.run("parse", *(paths[n] for n in names)))))
    for name in ("d1", "d101", "blanks_and_words"):
        ans, line = answers[name]
        assert ans is not None and _agrees(ans, _python(paths[name])), (name, line)
    assert answers["d1"][0][2].shape == (3, 1) and answers["d101"][0][2].shape == (4, 101)
    assert answers["blanks_and_words"][0][3] == 3                                        # " 1.5", "\tinf ", "-NaN"
    for name in ("header_only", "header_cut"):
        ans, line = answers[name]
        assert ans is not None and ans[0] == len(HEADER) and ans[1].size == 0, (name, line)
    for name, code, words in (("empty_line", -1, "line 3"), ("empty_line_crlf", -1, "line 3"), ("short_row", -1, "line 3"),
                              ("long_row", -1, "line 3"), ("quote", -5, "line 2 field 1"), ("bare_cr", -1, "line 2 field 1"),
                              ("no_value", -1, "line 2"), ("clip_text", -1, "line 2 field 0"), ("garbage_field", -1, "line 3 field 2"),
                              ("empty_file", -1, "line 1")):
        ans, line = answers[name]
        assert ans is None and line.startswith("error %d " % code) and words in line, (name, line)
    # the index itself: offsets of the lines, n + 1 of them
    idx = cd.run("index", paths["d1"]).strip().split("\n")
    assert idx[1].startswith("ok header_bytes %d rows 3 dim 1" % len(HEADER))
    offs = [int(ln.split()[1]) for ln in idx[2:5]] + [int(idx[5].split()[1])]
    data = cases["d1"]
    assert offs[0] == len(HEADER) + 1 and offs[-1] == len(data)
    assert [data[a:b] for a, b in zip(offs, offs[1:])] == data[len(HEADER) + 1:].splitlines(keepends=True)


def test_damaged_files_agree_with_python_or_are_refused(tmp_path):
    """300 seeded mutations of a small file, past the header line: overwrites (bytes that mean something to a CSV reader, or any byte)
    and truncations.  Whatever the driver accepts, the reference's reader accepts with the same clip numbers and the same bits."""
    rng = np.random.default_rng(5)
    base = HEADER + b"\n" + _rows(rng, 6, 5)[0]
    base_crlf = base.replace(b"\n", b"\r\n")
    alphabet = b"0123456789.,eE+-\n\r\" \tx_naif"
    paths = []
    for it in range(300):
        data = bytearray(base if it % 4 else base_crlf)
        lo = data.index(b"\n") + 1
        if it % 3 == 2:
            data = data[:int(rng.integers(lo, len(data)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                p = int(rng.integers(lo, len(data)))
                data[p] = alphabet[int(rng.integers(0, len(alphabet)))] if rng.random() < 0.8 else int(rng.integers(0, 256))
        paths.append(str(tmp_path / ("m%03d.csv" % it)))
        with open(paths[-1], "wb") as f:
            f.write(bytes(data))
    answers = _parse_answers(cd.run("parse", *paths))
    assert len(answers) == 300
    accepted = 0
    for path, (ans, line) in zip(paths, answers):
        if ans is None:
            assert "line " in line, line
            continue
        accepted += 1
        with open(path, "rb") as f:
            assert _agrees(ans, _python(path)), (f.read(), line)
    print("accepted %d of 300" % accepted)
    assert 30 <= accepted < 300


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(vq_\w+)\s*\(", text, flags=re.M)))


def test_csv_header_library_and_ctypes_table_agree():
    import video_query_algorithms_amd as vqa
    names = _declared("vq_amd_csv.h")
    assert names == ["vq_csv_index", "vq_db_load_csv"]
    assert sorted(vqa._lib.CSV_SIGNATURES) == names
    lib = vqa.load_library()
    raw = ctypes.CDLL(vqa._lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "vq_amd_csv.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    ctype_of = {"const char*": ctypes.c_char_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int64_t*": ctypes.POINTER(ctypes.c_int64),
                "int32_t*": ctypes.POINTER(ctypes.c_int32), "vq_db*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p}
    for name in names:
        assert hasattr(raw, name), "libvqamd.so does not export %s" % name
        assert getattr(lib, name).argtypes == vqa._lib.CSV_SIGNATURES[name]
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        types = [" ".join(p.split()[:-1]) for p in proto.split(",")]
        assert len(types) == len(vqa._lib.CSV_SIGNATURES[name]), name
        for t, bound in zip(types, vqa._lib.CSV_SIGNATURES[name]):
            assert bound in (ctype_of[t], ctypes.c_void_p), (name, t, bound)      # an output array may be bound as a plain pointer
    assert not set(names) & set(_declared("vq_amd.h")) and lib.vq_abi_version() == 12 and not set(names) & set(vqa._lib.exported_symbols())


def test_the_main_header_brings_the_csv_reader_along_in_plain_c():
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        assert '#include "vq_amd_csv.h"' in f.read()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "vq_amd.h"\nint main(void){ int (*f)(vq_db*, const char*, int64_t, int32_t, int32_t, const int64_t*, int64_t, int64_t, int64_t*) '
                    '= vq_db_load_csv; int (*g)(const char*, int64_t, int64_t, int64_t*, int64_t*, int32_t*, int64_t*, int64_t*) = vq_csv_index; '
                    '(void)f; (void)g; return VQ_OK; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "t.o")])


def test_index_features_reads_what_read_features_reads(tmp_path):
    from video_query_algorithms_amd import VqError
    from video_query_algorithms_amd.tsn import feature_csv
    rng = np.random.default_rng(2)
    body, _x = _rows(rng, 5, 8)
    path = str(tmp_path / "a.csv")
    with open(path, "wb") as f:
        f.write(HEADER + b"\n" + body)
    meta, clips, feats = feature_csv.read_features(path)
    for arg in (path, HEADER + b"\n" + body):
        m2, c2, dim, n = feature_csv.index_features(arg)
        assert m2 == meta and (c2 == clips).all() and c2.dtype == np.int64 and (dim, n) == feats.shape[::-1]
    with pytest.raises(VqError, match="line 3"):
        feature_csv.index_features(HEADER + b"\n1,0.5\n\n")
