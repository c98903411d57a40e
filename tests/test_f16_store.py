"""CPU: float16 in the binary feature store and the host-side conversion every fp16 route shares (feature_store.to_float16)."""
import json
import os
import re

import numpy as np
import pytest

from _helpers import reference_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def test_store_round_trip_keeps_dtype_and_bits(tmp_path):
    from video_query_algorithms_amd.feature_store import open_store, save_store
    rng = np.random.default_rng(0)
    x = (rng.random((9, 2, 3, 16)) * 70).astype(np.float16)
    x[0, 0, 0, :4] = [0.0, 6.0e-8, 6.1e-5, 65504.0]                      # zero, the smallest subnormal, the smallest normal, the largest
    present = np.ones((9, 2, 3), dtype=np.uint8)
    present[4, 1, 2] = 0
    path = save_store(str(tmp_path / "s"), x, np.arange(101, 110), ["rgb", "warped_optical_flow"], [1, 2, 3], present=present)
    meta, feats, ids, pres = open_store(path)
    assert meta["dtype"] == "float16" and feats.dtype == np.float16 and feats.shape == x.shape
    assert (_bits(np.asarray(feats)) == _bits(x)).all() and (ids == np.arange(101, 110)).all() and (np.asarray(pres) == present).all()
    with open(os.path.join(path, "meta.json")) as f:
        assert json.load(f)["dtype"] == "float16"
    with pytest.raises(ValueError):
        save_store(str(tmp_path / "bad"), x.astype(np.int16), np.arange(9), ["a", "b"], [1, 2, 3])


def test_store_from_the_reference_csv_tree_in_float16(tmp_path):
    from video_query_algorithms_amd.feature_store import open_store, store_from_csv_tree
    src = reference_features(str(tmp_path / "features"))
    for sub in sorted(os.listdir(src)):
        tree = os.path.join(src, sub)
        s64 = store_from_csv_tree(tree, str(tmp_path / (sub + "_64")), dtype=np.float64)
        s16 = store_from_csv_tree(tree, str(tmp_path / (sub + "_16")), dtype=np.float16)
        m16, f16, ids16, p16 = open_store(s16)
        _m64, f64, ids64, p64 = open_store(s64)
        assert m16["dtype"] == "float16" and f16.dtype == np.float16 and (ids16 == ids64).all()
        assert (p16 is None) == (p64 is None) and (p16 is None or (np.asarray(p16) == np.asarray(p64)).all())
        assert (_bits(np.asarray(f16)) == _bits(np.asarray(f64).astype(np.float16))).all()      # the fp64 values rounded once
        assert np.isfinite(np.asarray(f16, dtype=np.float32)).all()


def test_overflow_is_refused_with_the_first_offending_index():
    from video_query_algorithms_amd.feature_store import to_float16
    x = np.ones((3, 2, 1, 4))
    x[1, 1, 0, 2] = 70000.0
    x[2, 0, 0, 0] = -1e9
    with pytest.raises(ValueError, match=r"70000.*\(1, 1, 0, 2\)"):
        to_float16(x)
    with pytest.raises(ValueError):
        to_float16(np.float32([65520.0]))                                  # the tie above the largest half rounds to infinity
    ok = to_float16(np.array([65519.0, -65504.0, np.inf, 1e-8, 2.0 ** -25 * 1.5]))
    assert ok.dtype == np.float16 and ok[0] == 65504.0 and ok[1] == -65504.0 and np.isinf(ok[2])   # an infinity that was one stays
    assert ok[3] == 0.0 and ok[4] == np.float16(2.0 ** -24)                # underflow is rounding, not an error
    h = np.float16([1.5, 3.0])
    assert to_float16(h) is h


def test_store_from_csv_tree_refuses_values_no_half_can_hold(tmp_path):
    from video_query_algorithms_amd.feature_store import store_from_csv_tree
    src = reference_features(str(tmp_path / "features"))
    tree = os.path.join(src, sorted(os.listdir(src))[0])
    victim = None
    for dirpath, _d, files in os.walk(tree):
        for fn in files:
            if fn.endswith(".csv"):
                victim = os.path.join(dirpath, fn)
    with open(victim) as f:
        lines = f.read().split("\n")
    cells = lines[1].split(",")                                           # line 0 is the file's header
    cells[3] = "123456.0"
    lines[1] = ",".join(cells)
    with open(victim, "w") as f:
        f.write("\n".join(lines))
    store_from_csv_tree(tree, str(tmp_path / "s32"), dtype=np.float32)    # float32 holds it
    with pytest.raises(ValueError, match="float16"):
        store_from_csv_tree(tree, str(tmp_path / "s16"), dtype=np.float16)


def test_the_enum_value_is_two_in_the_header_and_the_binding():
    from video_query_algorithms_amd import _lib
    assert (_lib.VQ_F32, _lib.VQ_F64, _lib.VQ_F16) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        header = f.read()
    assert re.search(r"enum\s*\{\s*VQ_F32\s*=\s*0\s*,\s*VQ_F64\s*=\s*1\s*,\s*VQ_F16\s*=\s*2\s*\}", header)
    assert "#define VQ_ABI_VERSION 12" in header or re.search(r"VQ_ABI_VERSION\s+12", header)
