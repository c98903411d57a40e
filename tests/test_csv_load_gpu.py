"""GPU: feature CSV files parsed on the device into a resident database (vq_db_load_csv, FeatureDB.load_csv / from_csv_tree).

Every comparison is bit for bit: the device converts decimal text to the correctly rounded binary64 (what float() returns) and rounds
once to the database's type (what numpy's astype does), so there is one right answer per element and no tolerance.

A database's D is a multiple of 4 (vq_db_create), so the widths here are 4, 8, 100, 1024 and 2048; D = 1 and D = 101 FILES go through
the same shared arithmetic and the indexer on the host (tests/test_csv_index_host.py) -- no database of that width can exist."""
import os

import numpy as np
import pytest

import _csv_driver as cd
from _helpers import reference_features

pytestmark = pytest.mark.gpu
HEADER = b"video =v, video url =/a/v.mp4, CNN stream =rgb, feature blob =global_pool, caffe model =m.caffemodel\n"


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _zero_db(vqa, n, s, e, d, dtype):
    db = vqa.FeatureDB(n, s, e, d, dtype=dtype)
    db.upload(0, np.zeros((n, s, e, d), dtype=dtype))
    return db


def test_hard_values_and_the_fields_the_host_resolves(vqa):
    slow = cd.SLOW + ["-Infinity", "1.5 "]
    cells = cd.HARD + slow + ["%r" % v for v in np.random.default_rng(0).standard_normal(40 - len(cd.HARD) - len(slow)).tolist()]
    assert len(cells) == 40
    text = HEADER + "".join("%d,%s\n" % (r + 1, ",".join(cells[8 * r:8 * r + 8])) for r in range(5)).encode()
    want = np.array([float(c) for c in cells]).reshape(5, 8)
    db = _zero_db(vqa, 5, 1, 1, 8, np.float64)
    host = db.load_csv(text, 0, 0, np.arange(5))
    got = db.read_rows(np.arange(5)).reshape(5, 8)
    assert (_u(got) == _u(want)).all(), (got, want)
    assert host == len(slow)
    # the same text into float32: one rounding from the double; the values no float holds become inf like astype's
    db32 = _zero_db(vqa, 5, 1, 1, 8, np.float32)
    db32.load_csv(text, 0, 0, np.arange(5))
    with np.errstate(over="ignore"):
        assert (_u(db32.read_rows(np.arange(5)).reshape(5, 8)) == _u(want.astype(np.float32))).all()


@pytest.mark.parametrize("fmt", ["repr", "g12"])
@pytest.mark.parametrize("n,d", [(3, 4), (70, 100), (3, 2048)])
def test_files_of_the_formatter_in_both_number_formats(vqa, n, d, fmt):
    from video_query_algorithms_amd.tsn import feature_csv
    rng = np.random.default_rng(d)
    x = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-300 if d == 2048 else -12, 12, (n, d))       # D = 2048: the longest lines there are
    x[0, 0], x[n - 1, d - 1] = 0.0, -1.5e-310
    body = feature_csv.format_rows(x, np.arange(1, n + 1), fmt)
    want = x if fmt == "repr" else np.array([[float(c) for c in ln.split(",")[1:]] for ln in body.decode().splitlines()])
    for dtype in (np.float64, np.float32):
        db = _zero_db(vqa, n, 1, 1, d, dtype)
        assert db.load_csv(HEADER + body, 0, 0, np.arange(n)) == 0
        with np.errstate(over="ignore", under="ignore"):
            assert (_u(db.read_rows(np.arange(n)).reshape(n, d)) == _u(want.astype(dtype))).all()


@pytest.fixture(scope="module")
def golden_trees(tmp_path_factory):
    src = reference_features(str(tmp_path_factory.mktemp("features")))
    return [os.path.join(src, sub) for sub in sorted(os.listdir(src))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16])
def test_the_shipped_trees_equal_the_store_route(vqa, golden_trees, tmp_path, dtype):
    from video_query_algorithms_amd.feature_store import open_store, store_from_csv_tree
    assert len(golden_trees) == 2
    for k, tree in enumerate(golden_trees):
        store = store_from_csv_tree(tree, str(tmp_path / ("s%d" % k)), dtype=dtype)
        meta, feats, ids, present = open_store(store)
        via_store = vqa.FeatureDB.from_store(store)
        db = vqa.FeatureDB.from_csv_tree(tree, dtype=dtype)
        assert db.dtype == np.dtype(dtype) and (db.n, db.S, db.E, db.D) == feats.shape
        assert db.read_rows(np.arange(db.n)).tobytes() == np.ascontiguousarray(feats).tobytes()
        assert (db.clip_ids == ids).all() and (db.clip_ids == via_store.clip_ids).all()
        assert (db.present is None) == (present is None) and (present is None or (db.present == np.asarray(present)).all())
        assert db.stream_names == via_store.stream_names and db.slot_splits == via_store.slot_splits
        assert db.csv_host_fields == 0
        import json
        with open(os.path.join(store, "clips.json")) as f:
            assert db.clips == [(c["video"], c["clip"]) for c in json.load(f)]
        db.close()
        via_store.close()


def test_a_value_no_half_holds_is_refused_in_float16_only(vqa, golden_trees):
    tree = golden_trees[0]
    victim = None
    for dirpath, _d, files in os.walk(tree):
        for fn in files:
            if fn.endswith(".csv"):
                victim = os.path.join(dirpath, fn)
    with open(victim) as f:
        original = f.read()
    lines = original.split("\n")
    cells = lines[1].split(",")                                           # line 0 is the file's header
    cells[3] = "123456.0"
    lines[1] = ",".join(cells)
    try:
        with open(victim, "w") as f:
            f.write("\n".join(lines))
        db = vqa.FeatureDB.from_csv_tree(tree, dtype=np.float32)          # float32 holds it
        assert db.csv_host_fields == 0
        with pytest.raises(ValueError, match=r"(?s)%s.*line 2 field 3.*float16" % os.path.basename(victim)):
            vqa.FeatureDB.from_csv_tree(tree, dtype=np.float16)
    finally:
        with open(victim, "w") as f:
            f.write(original)


@pytest.fixture(scope="module")
def wide_file():
    """20 clips of D = 1024 as one file's bytes, the float64 values it reads as, and the rows it is loaded through."""
    from video_query_algorithms_amd.tsn import feature_csv
    rng = np.random.default_rng(11)
    x = (rng.random((20, 1024)).astype(np.float32) * np.float32(4.0)).astype(np.float64)
    x[3, 5] = 1e-7
    text = HEADER + feature_csv.format_rows(x, np.arange(1, 21), "repr")
    rows = rng.permutation(24)[:20].astype(np.int64)
    rows[[4, 17]] = -1
    return text, x, rows


def _expected(x, rows, n=24, s=2, e=3, slot=(1, 2)):
    want = np.zeros((n, s, e, x.shape[1]), dtype=np.float32)
    for i, r in enumerate(rows.tolist()):
        if r >= 0:
            want[r, slot[0], slot[1]] = x[i].astype(np.float32)
    return want


def test_permuted_rows_into_both_layouts_and_a_scan_afterwards(vqa, wide_file):
    text, x, rows = wide_file
    want = _expected(x, rows)
    got, scores = {}, {}
    t = np.random.default_rng(1).random((2, 3, 1024))
    for layout in ("rows", "tiled", "uploaded"):
        db = _zero_db(vqa, 24, 2, 3, 1024, np.float32)
        if layout == "tiled":
            db.set_layout("tiled")
        if layout == "uploaded":
            db.upload(0, want)
        else:
            assert db.load_csv(text, 1, 2, rows) == 0
        if layout == "tiled":
            assert db.layout == "tiled"
            inside = db.read_rows(np.arange(24))
            assert inside.tobytes() == want.tobytes()
            db.set_layout("rows")
        got[layout] = db.read_rows(np.arange(24))
        db.set_query(t)
        db.scan(weights=[1.0, 1.5])
        scores[layout] = db.scores()
        db.close()
    assert got["rows"].tobytes() == want.tobytes() and got["tiled"].tobytes() == want.tobytes()      # untouched rows and slots stay zero
    assert (_u(scores["rows"]) == _u(scores["uploaded"])).all() and (_u(scores["tiled"]) == _u(scores["uploaded"])).all()


def test_chunk_sizes_give_identical_bytes(vqa, wide_file):
    text, x, rows = wide_file
    want = _expected(x, rows)
    line = len(text.split(b"\n")[1]) + 1
    for chunk in (1, line + line // 2, len(text)):
        db = _zero_db(vqa, 24, 2, 3, 1024, np.float32)
        assert db.load_csv(text, 1, 2, rows, chunk_bytes=chunk) == 0
        assert db.read_rows(np.arange(24)).tobytes() == want.tobytes(), chunk
        db.close()


def test_refusals_store_nothing_and_a_garbage_field_is_named(vqa, wide_file):
    text, x, rows = wide_file
    db = _zero_db(vqa, 24, 2, 3, 1024, np.float32)
    twice = rows.copy()
    twice[0] = twice[1]
    outside = rows.copy()
    outside[0] = 24
    narrow = HEADER + b"1,0.5,0.25,0.125,1.0\n" * 20
    for args, words in (((text, 1, 2, twice), "twice"), ((text, 1, 2, outside), "outside"), ((narrow, 1, 2, rows), "values"),
                        ((text, 1, 2, rows[:19]), "data rows"), ((text, 2, 0, rows), "slot")):
        with pytest.raises(vqa.VqError, match=words) as ei:
            db.load_csv(*args)
        assert ei.value.code == -1
    assert not db.read_rows(np.arange(24)).any()
    lines = text.split(b"\n")
    cells = lines[20].split(b",")                                         # the last data row: line 21 of the file
    cells[1000] = b"0.5x7"
    lines[20] = b",".join(cells)
    with pytest.raises(vqa.VqError, match="line 21 field 1000.*0.5x7") as ei:
        db.load_csv(b"\n".join(lines), 1, 2, rows)
    assert ei.value.code == -1
    db.close()


def test_more_host_fields_than_the_list_holds_are_all_resolved(vqa):
    """70 x 1024 fields the device hands back (a leading blank) are more than the 65536 entries of its list: the chunk is run again in
    pieces that cannot overflow it, and every field arrives."""
    rng = np.random.default_rng(9)
    x = np.round(rng.random((70, 1024)) * 8.0, 3)
    text = HEADER + "".join("%d,%s\n" % (i + 1, ",".join(" %r" % v for v in row)) for i, row in enumerate(x.tolist())).encode()
    db = _zero_db(vqa, 70, 1, 1, 1024, np.float64)
    assert db.load_csv(text, 0, 0, np.arange(70)) == 70 * 1024
    assert (_u(db.read_rows(np.arange(70)).reshape(70, 1024)) == _u(x)).all()
    db.close()


def test_written_features_come_back_with_their_bits(vqa, tmp_path):
    """64 clips of float32-mean features (calcSig_wOF.py:82) written by write_features and loaded by from_csv_tree(dtype=float64)."""
    from video_query_algorithms_amd.tsn import feature_csv
    rng = np.random.default_rng(64)
    feats = {m: (rng.random((64, 25, 1024)).astype(np.float32) * np.float32(2.0)).astype(np.float64).mean(axis=1) for m in feature_csv.STREAM_MODES}
    names = ["clip_%04d" % (i + 1) for i in range(64)]
    for split in (1, 2):
        feature_csv.write_features(str(tmp_path / "features"), "video_a", "/a/video_a.mp4", "UCF101_split%d" % split, "global_pool", names,
                                   feats, {m: m + ".caffemodel" for m in feature_csv.STREAM_MODES})
    db = vqa.FeatureDB.from_csv_tree(str(tmp_path / "features"), dtype=np.float64)
    assert (db.n, db.S, db.E, db.D) == (64, 2, 2, 1024) and db.present is None and db.csv_host_fields == 0
    got = db.read_rows(np.arange(64))
    for si, m in enumerate(feature_csv.STREAM_MODES):
        for ei in range(2):
            assert (_u(got[:, si, ei]) == _u(feats[m])).all()
    assert db.clips == [("video_a", i + 1) for i in range(64)] and db.slot_splits == [[1, 2], [1, 2]]
    tiled = vqa.FeatureDB.from_csv_tree(str(tmp_path / "features"), dtype=np.float32, layout="tiled")       # the values land in their tiles
    assert tiled.layout == "tiled"
    got32 = tiled.read_rows(np.arange(64))
    for si, m in enumerate(feature_csv.STREAM_MODES):
        for ei in range(2):
            assert (_u(got32[:, si, ei]) == _u(feats[m].astype(np.float32))).all()
