"""Quick device-side timing of the similarity scan (HIP events through the C ABI)."""
import ctypes as C
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import video_query_algorithms_amd as vqa
from video_query_algorithms_amd._lib import call


def bench(n, s, e, d=1024, reps=10, dtype=np.float32):
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=1, scales=(4.0, 1.0)[:s], dtype=dtype)
    db.set_query_from_row(7, want=False)
    w = [1.0, 1.5][:s]
    db.scan(weights=w)
    tm = C.c_void_p()
    call("vq_timer_create", C.byref(tm))
    times = []
    for _ in range(reps):
        call("vq_timer_start", tm, None)
        db.scan(weights=w)
        call("vq_timer_stop", tm, None)
        ms = C.c_float()
        call("vq_timer_elapsed_ms", tm, C.byref(ms))
        times.append(ms.value)
    nbytes = n * s * e * d * np.dtype(dtype).itemsize + n * 8
    best, med = min(times), sorted(times)[len(times) // 2]
    print("N=%d S=%d E=%d %s: %.3f ms median (%.3f best) -> %.1f GB/s median, %.1f GB/s best (%.2f of 8 TB/s)"
          % (n, s, e, np.dtype(dtype).name, med, best, nbytes / med / 1e6, nbytes / best / 1e6, nbytes / med / 1e6 / 8000),
          flush=True)
    db.close()


if __name__ == "__main__" and len(sys.argv) == 1:
    bench(200_000, 2, 5)
    bench(300_000, 2, 3)
    bench(10_000, 2, 3)
    bench(100_000, 2, 5, dtype=np.float64)
    bench(1_000_000, 2, 5)
    bench(10_000, 2, 3, dtype=np.float16)
    bench(1_000_000, 2, 5, dtype=np.float16)


def bench_batched(n=1_000_000, s=2, e=5, d=1024, q=16, reps=6, dtype=np.float32):
    """vq_db_scan_batch at cfg 4 (the fused single launch), three timed repeats."""
    import time
    db = vqa.FeatureDB.synthetic(n, s, e, d, seed=17, scales=(4.0, 1.0)[:s], dtype=dtype)
    rng = np.random.default_rng(0)
    t = rng.standard_normal((q, s, e, d)) / d
    w = 0.5 + rng.random((q, s))
    for form in ("fused", "fused", "fused"):
        db.scan_batch(t, w, want=False)
        db.scores_sync() if hasattr(db, "scores_sync") else db.scan_batch(t[:1], w[:1])     # drain
        tm = C.c_void_p()
        call("vq_timer_create", C.byref(tm))
        times = []
        for _ in range(reps):
            call("vq_timer_start", tm, None)
            db.scan_batch(t, w, want=False)
            call("vq_timer_stop", tm, None)
            ms = C.c_float()
            call("vq_timer_elapsed_ms", tm, C.byref(ms))
            times.append(ms.value)
        med = sorted(times)[len(times) // 2]
        dbb = n * s * e * d * np.dtype(dtype).itemsize
        print("batched Q=%d %s %s: %.3f ms median (%.3f best) -> %.0f queries/s, DB bytes %.2f TB/s (%.3f of 8 TB/s)"
              % (q, np.dtype(dtype).name, "two-kernel" if form == "1" else "fused", med, min(times), q / med * 1e3, dbb / med / 1e9, dbb / med / 1e9 / 8), flush=True)
    db.close()


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "batched":
    bench_batched()
    bench_batched(dtype=np.float16)


def _timed_scan(db, w, tm):
    call("vq_timer_start", tm, None)
    db.scan(weights=w)
    call("vq_timer_stop", tm, None)
    ms = C.c_float()
    call("vq_timer_elapsed_ms", tm, C.byref(ms))
    return ms.value


def bench_view(n=1_000_000, s=2, e=5, d=1024, frac=10, run=100, reps=40, dtype=np.float32):
    """The scan over a search set of M = N / frac rows of an N-row database, against the scan of a plain M-row database on the same
    box (what a database per search set costs): one contiguous run; runs of `run` rows (a video) spread evenly; the same runs on the
    tiled layout.  The two handles are timed in turn, `reps` times; medians.  GB/s counts the bytes the M clips NEED (their rows and
    their scores), not what a tiled scan reads of the tiles it touches."""
    m = n // frac
    w = [1.0, 1.5][:s]
    big = vqa.FeatureDB.synthetic(n, s, e, d, seed=1, scales=(4.0, 1.0)[:s], dtype=dtype)
    small = vqa.FeatureDB.synthetic(m, s, e, d, seed=1, scales=(4.0, 1.0)[:s], dtype=dtype)
    for db in (big, small):
        db.set_query_from_row(7, want=False)
    starts = (np.arange(m // run) * (n // (m // run))).astype(np.int64)
    runs = (starts[:, None] + np.arange(run)[None, :]).reshape(-1)
    big.define_search_rows("contiguous", np.arange(n // 3, n // 3 + m))
    big.define_search_rows("runs", runs)
    need = m * s * e * d * np.dtype(dtype).itemsize + m * 8
    tm = C.c_void_p()
    call("vq_timer_create", C.byref(tm))
    print("view scan, N=%d M=%d S=%d E=%d %s (%d timed scans each, in turn with the plain M-row database)" % (n, m, s, e, np.dtype(dtype).name, reps), flush=True)
    for layout, name in (("rows", "contiguous"), ("rows", "runs"), ("tiled", "runs")):
        big.use_search_set(None)
        big.set_layout(layout)
        big.use_search_set(name)
        for db in (big, small):
            for _ in range(3):
                db.scan(weights=w)
        tv, tp = [], []
        for _ in range(reps):
            tp.append(_timed_scan(small, w, tm))
            tv.append(_timed_scan(big, w, tm))
        mv, mp = sorted(tv)[reps // 2], sorted(tp)[reps // 2]
        touched = np.unique(big.use_search_set(name).rows >> 4).size * 16 if layout == "tiled" else m
        print("  %-5s %-10s: view %.3f ms (best %.3f), plain M-row database %.3f ms (best %.3f): ratio %.3f; %.0f GB/s of needed bytes (%.2f of 8 TB/s), "
              "reads %.2f x the rows needed" % (layout, name if name == "contiguous" else "runs of %d" % run, mv, min(tv), mp, min(tp), mv / mp,
                                                need / mv / 1e6, need / mv / 1e6 / 8000, touched / m), flush=True)
    big.close()
    small.close()


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "view":
    bench_view(s=2, e=5)
    bench_view(s=2, e=3)


def _timed(fn, tm):
    call("vq_timer_start", tm, None)
    fn()
    call("vq_timer_stop", tm, None)
    ms = C.c_float()
    call("vq_timer_elapsed_ms", tm, C.byref(ms))
    return ms.value


MATRIX_MS_PER_ELEMENT = 4.2 / 10.24e9       # csrc/vq_sim_batch.hip: 16 queries x 10.24 G elements are 4.2 ms of fp64 matrix time


def bench_layout(layout, dtype, n=1_000_000, s=2, e=3, d=1024, q=16, reps=12, out=None, note=None):
    """A database on its rows against the same database in its tiled layout (``layout``: "tiled64" for float64, "tiled16" for
    float16), in ONE process: two handles of the same seed, timed in turn (bench_view's pattern) behind a warm-up, `reps` (>= 10) times
    each -- the one-query scan, then the 16-query pass.  GB/s is the algorithmic bytes (the rows + 8 B of score per clip) over
    device-event time; the share is of 8 TB/s; the pass is also put against its fp64 matrix time.  The row-major figures of the same run
    are the baseline.  ``out``: a JSON file with every sample; ``note``: what the run is (e.g. the group size the library was built with)."""
    import json
    import time
    assert reps >= 10
    w = [1.0, 1.5][:s]
    rows = vqa.FeatureDB.synthetic(n, s, e, d, seed=1, scales=(4.0, 1.0)[:s], dtype=dtype)
    tiled = vqa.FeatureDB.synthetic(n, s, e, d, seed=1, scales=(4.0, 1.0)[:s], dtype=dtype)
    t0 = time.perf_counter()
    tiled.set_layout(layout)                         # synchronous: one sweep of the block each way through 256 MB of scratch
    convert_ms = (time.perf_counter() - t0) * 1e3
    assert tiled.layout == layout and rows.layout == "rows"
    handles = (("rows", rows), (layout, tiled))
    size, kind = np.dtype(dtype).itemsize, np.dtype(dtype).name
    for _name, db in handles:
        db.set_query_from_row(7, want=False)
    tm = C.c_void_p()
    call("vq_timer_create", C.byref(tm))
    nbytes = n * s * e * d * size + n * 8
    res = {"n": n, "S": s, "E": e, "D": d, "dtype": kind, "layout": layout, "note": note, "bytes": nbytes, "reps": reps, "convert_ms": convert_ms,
           "scan": {}, "batch": {}}
    print("%s N=%d S=%d E=%d (%.1f GB): rows -> %s in %.0f ms (%.2f TB/s of the block, read + written once each)%s"
          % (kind, n, s, e, nbytes / 1e9, layout, convert_ms, 2 * nbytes / convert_ms / 1e9, " [%s]" % note if note else ""), flush=True)
    for _name, db in handles:
        for _ in range(3):
            db.scan(weights=w)
    times = {name: [] for name, _db in handles}
    for _ in range(reps):
        for name, db in handles:
            times[name].append(_timed(lambda: db.scan(weights=w), tm))
    for name, _db in handles:
        med, best = sorted(times[name])[reps // 2], min(times[name])
        res["scan"][name] = {"ms": times[name], "median_ms": med, "best_ms": best, "median_gbs": nbytes / med / 1e6, "best_gbs": nbytes / best / 1e6,
                             "median_share_of_8tbs": nbytes / med / 1e6 / 8000}
        print("  one-query scan %-7s: %.3f ms median (%.3f best) -> %.0f GB/s median, %.0f best (%.3f of 8 TB/s)"
              % (name, med, best, nbytes / med / 1e6, nbytes / best / 1e6, nbytes / med / 1e6 / 8000), flush=True)
    rng = np.random.default_rng(0)
    t = rng.standard_normal((q, s, e, d)) / d
    wq = 0.5 + rng.random((q, s))
    first = {}
    for name, db in handles:
        first[name] = db.scan_batch(t, wq)              # warm-up, drained by the copy back
        db.scan_batch(t, wq, want=False)
        db.scan_batch(t[:1], wq[:1])
    assert (first["rows"] == first[layout]).all()       # the same bits: what is timed is the same computation
    times = {name: [] for name, _db in handles}
    for _ in range(reps):
        for name, db in handles:
            times[name].append(_timed(lambda: db.scan_batch(t, wq, want=False), tm))
    dbb = n * s * e * d * size
    matrix_ms = MATRIX_MS_PER_ELEMENT * n * s * e * d * (q / 16)
    for name, _db in handles:
        med, best = sorted(times[name])[reps // 2], min(times[name])
        res["batch"][name] = {"ms": times[name], "median_ms": med, "best_ms": best, "queries_per_s": q / med * 1e3, "median_share_of_8tbs": dbb / med / 1e6 / 8000,
                              "matrix_ms": matrix_ms, "median_over_matrix_ms": med / matrix_ms}
        print("  16-query pass  %-7s: %.3f ms median (%.3f best) -> %.0f queries/s, DB bytes %.2f TB/s (%.3f of 8 TB/s), %.2f x the %.2f ms of matrix time"
              % (name, med, best, q / med * 1e3, dbb / med / 1e9, dbb / med / 1e9 / 8, med / matrix_ms, matrix_ms), flush=True)
    rows.close()
    tiled.close()
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    return res


def bench_tiled64(n=1_000_000, s=2, e=3, **kw):
    return bench_layout("tiled64", np.float64, n, s, e, **kw)


def bench_tiled16(n=1_000_000, s=2, e=5, **kw):
    """float16 rows against tiled16.  The group-size A/B (VQ_TILED_GROUP16 = 2 / 4 / 8) is this mode once per library: build the
    library with VQ_EXTRA_HIPCC_FLAGS=-DVQ_TILED_GROUP16=<g> into a file of its own, point VQ_AMD_LIB at it and pass the value as the note."""
    return bench_layout("tiled16", np.float16, n, s, e, **kw)


def bench_short(n, dtype, s=2, e=3, d=101, alternations=4, reps=10, seed=1):
    """scan_short_kernel against scan_generic_kernel on the same rows of logical length ``d`` (stored at d rounded up to a multiple of
    4), in one process: two handles of the same data, one created with VQ_DIM_SHORT_ROWS and one with VQ_DIM_PADDED alone
    (include/vq_amd_dim.h; the environment is not touched), timed in turn -- ``alternations`` (>= 3) blocks of ``reps`` scans each,
    behind a warm-up of both.  The generic kernel is the baseline: what a hand-padded plain database runs.  Per kernel: the median of
    each block, the median and the spread (max - min) of those block medians, GB/s and the share of 8 TB/s over the bytes stored (pads
    included: they are read) plus 8 B of score per clip.  The two kernels must agree to 1e-12 on what they computed here."""
    assert alternations >= 3
    size = np.dtype(dtype).itemsize
    handles = (("generic", vqa.FeatureDB(n, s, e, d, dtype=dtype, short_rows=False)), ("short", vqa.FeatureDB(n, s, e, d, dtype=dtype, short_rows=True)))
    rng = np.random.default_rng(seed)
    chunk = max(1, (256 << 20) // (s * e * d * 4))
    for r in range(0, n, chunk):
        k = min(chunk, n - r)
        x = np.abs(rng.standard_normal((k, s, e, d), dtype=np.float32)).astype(dtype)
        for _name, db in handles:
            db.upload(r, x)
    w = [1.0, 1.5][:s]
    tm = C.c_void_p()
    call("vq_timer_create", C.byref(tm))
    first = {}
    for name, db in handles:
        db.set_query_from_row(7, want=False)
        for _ in range(3):
            db.scan(weights=w)
        first[name] = db.scores()
    agree = float(np.abs(first["short"] - first["generic"]).max())
    assert agree <= 1e-12, agree
    blocks = {name: [] for name, _db in handles}
    for _ in range(alternations):
        for name, db in handles:
            ms = sorted(_timed(lambda: db.scan(weights=w), tm) for _ in range(reps))
            blocks[name].append(ms[reps // 2])
    pitch = handles[0][1].Dp
    nbytes = n * s * e * pitch * size + n * 8
    res = {"n": n, "S": s, "E": e, "d": d, "stored_D": pitch, "dtype": np.dtype(dtype).name, "bytes": nbytes, "alternations": alternations,
           "reps_per_block": reps, "max_abs_score_difference": agree, "kernels": {}}
    for name, _db in handles:
        b = blocks[name]
        med = sorted(b)[len(b) // 2]
        res["kernels"][name] = {"block_median_ms": b, "median_ms": med, "spread_ms": max(b) - min(b), "gbs": nbytes / med / 1e6,
                                "share_of_8tbs": nbytes / med / 1e6 / 8000}
        print("short-row A/B N=%d %dx%dx%d %s %-7s: %.4f ms (block medians %s, spread %.4f) -> %.0f GB/s (%.3f of 8 TB/s)"
              % (n, s, e, d, np.dtype(dtype).name, name, med, " ".join("%.4f" % v for v in b), max(b) - min(b), nbytes / med / 1e6,
                 nbytes / med / 1e6 / 8000), flush=True)
    g, sh = res["kernels"]["generic"], res["kernels"]["short"]
    res["short_faster_by_ms"] = g["median_ms"] - sh["median_ms"]
    res["short_wins_beyond_spread"] = bool(g["median_ms"] - sh["median_ms"] > max(g["spread_ms"], sh["spread_ms"]))
    for _name, db in handles:
        db.close()
    return res


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "short":
    # tools/quick_sim_bench.py short [out.json]: 10 000 and 1 000 000 clips x 2 x 3 x 101, float32 and float64
    import json
    results = [bench_short(n, dt) for n in (10_000, 1_000_000) for dt in (np.float32, np.float64)]
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump({"what": "scan_short_kernel (a handle with VQ_DIM_SHORT_ROWS) against scan_generic_kernel (VQ_DIM_PADDED alone) on the same rows, in turn",
                       "results": results}, f, indent=1)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] in ("tiled64", "tiled16"):
    # tools/quick_sim_bench.py tiled64|tiled16 [n s e [out.json [note]]]: one shape per process (each under a time limit of its own)
    a = sys.argv[2:]
    {"tiled64": bench_tiled64, "tiled16": bench_tiled16}[sys.argv[1]](*(int(v) for v in a[:3]), out=a[3] if len(a) > 3 else None,
                                                                      note=a[4] if len(a) > 4 else None)
