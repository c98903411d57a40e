"""CPU: the host-only translation units of the library (video-query-algorithms_amd/csrc/host/*.cc) under AddressSanitizer +
UndefinedBehaviorSanitizer and under ThreadSanitizer.

vq_jpeg_host.cc parses UNTRUSTED files on worker threads (markers, Huffman tables, restart markers, the host entropy decoder, the
unstuffing pass of the device decoder); vq_corners.cc selects corners on host threads; vq_block_pool.cc is a process-wide pool
shared by every extractor handle; vq_csv.cc writes text into caller-sized buffers; vq_tsn_plan.cc holds every check that stands
between a caller's layer plan and the device; vq_flow_host.cc is the flow handle's host arithmetic (pyramid sizes, tile cuts, launch
chunks, the fp64 homography algebra, the layout of its scratch blocks), judged below against the oracles.  GPU sanitizers are not available on the
pool, so these units are kept free of HIP and built here by tests/sanitize/Makefile with plain g++; tests/sanitize/san_driver.cc
drives them the way csrc/vq_jpeg.hip / vq_flow.hip / vq_tsn.hip do, with buffers of EXACTLY the sizes the product reserves.
The corpus: the committed JPEG fixtures (4:2:0 / 4:2:2 / 4:4:4 / grey, optimised tables, restart intervals, odd sizes) and
600 seeded mutations of them (overwritten bytes, truncations, 4-byte splices) -- the mutation test of tests/test_jpeg_gpu.py, which
runs un-instrumented on the GPU box."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINDINGS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "WARNING: ThreadSanitizer", "SUMMARY: ")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    out = str(tmp_path_factory.mktemp("san"))
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "sanitize"), "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return {k: os.path.join(out, "san_driver_" + k) for k in ("asan", "tsan")}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("corpus"))
    seeds = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jpg")))]
    assert len(seeds) >= 5
    for k, s in enumerate(seeds):
        with open(os.path.join(d, "seed_%02d.jpg" % k), "wb") as f:
            f.write(s)
    rng = np.random.default_rng(0)
    for it in range(600):
        base = bytearray(seeds[it % len(seeds)])
        if it % 3 == 0:
            for _ in range(int(rng.integers(1, 6))):
                base[int(rng.integers(2, len(base)))] = int(rng.integers(0, 256))
        elif it % 3 == 1:
            base = base[:int(rng.integers(4, len(base)))]
        else:
            p = int(rng.integers(2, len(base) - 8))
            base[p:p + 4] = bytes(rng.integers(0, 256, 4, dtype=np.uint8))
        with open(os.path.join(d, "mut_%03d.jpg" % it), "wb") as f:
            f.write(bytes(base))
    return d


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=0")
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert r.returncode == 0 and not any(tag in r.stdout for tag in FINDINGS), r.stdout[-4000:]
    return r.stdout


def test_every_damaged_file_alone_under_asan_ubsan(drivers, corpus):
    out = _run(drivers["asan"], "single", corpus)
    decoded, refused = (int(x.split()[0]) for x in out.split(":")[1].split(","))
    assert decoded > 100 and refused > 100, out            # both outcomes are exercised, as on the GPU box


def test_threaded_batch_stages_under_asan_and_tsan(drivers, corpus):
    for kind in ("asan", "tsan"):
        out = _run(drivers[kind], "batch", corpus)
        assert "batches decoded" in out and " 0 batches decoded" not in out, out


@pytest.mark.parametrize("mode", ["csv", "corners", "pool", "plan", "flow"])
def test_formatter_corner_selection_and_block_pool(drivers, mode):
    for kind in ("asan", "tsan"):
        assert mode + ": ok" in _run(drivers[kind], mode)


def test_host_entropy_decoder_gives_the_oracles_coefficients(drivers):
    """No GPU needed for this half of the JPEG path: csrc/host/vq_jpeg_host.cc:decode_scan (the decoder of the command line's RGB batches)
    against oracle/jpeg_oracle.py:decode_coefficients -- which is pinned against libjpeg-turbo -- on every committed fixture, as
    position-weighted sums per component."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import jpeg_oracle as jo
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jpg")))
    assert len(files) >= 5
    try:                                                   # with Pillow here: noise at quality 100 (an FF 00 every ~250 bytes, the longest codes)
        import io
        from PIL import Image
        rng = np.random.default_rng(5)
        for k, (h, w, sub) in enumerate(((40, 56, 2), (33, 47, 1), (24, 24, 0), (64, 80, 2))):
            buf = io.BytesIO()
            kw = {"restart_marker_blocks": 3} if k == 3 else {}
            try:
                Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, "JPEG", quality=100, subsampling=sub, **kw)
            except TypeError:
                continue
            path = os.path.join(os.path.dirname(drivers["asan"]), "noise_%d.jpg" % k)
            with open(path, "wb") as f:
                f.write(buf.getvalue())
            files.append(path)
    except ImportError:
        pass
    for path in files:
        data = open(path, "rb").read()
        try:
            _info, coef = jo.decode_coefficients(data)
        except jo.JpegError:
            continue                                       # a fixture the decoders refuse (progressive, ...)
        out = _run(drivers["asan"], "coef", path)
        lines = [ln for ln in out.splitlines() if ln.startswith("component")]
        assert len(lines) == len(coef), out
        for ln, c in zip(lines, coef):
            flat = c.reshape(-1).astype(np.int64)
            w = np.arange(flat.size, dtype=np.int64) % 65521 + 1
            want = "%d x %d blocks, sums %d %d" % (c.shape[0], c.shape[1], int(flat.sum()), int((flat * w).sum()))
            assert ln.endswith(want), (path, ln, want)


def _numbers(line, tag):
    assert line.startswith(tag + " "), (tag, line)
    return [float(v) for v in line[len(tag):].split()]


def test_flow_host_arithmetic_against_the_oracles(drivers, tmp_path):
    """csrc/host/vq_flow_host.cc through `san_driver flow <file>` (a case per line in, a result per line out as %.17g), under ASan + UBSan.
    Bars: pyramid sizes and tile cuts EQUAL (oracle/tvl1_oracle.py; the cuts the parent commit's library named on an MI355X,
    tests/golden/flow_plan/tile_cuts.json, which also satisfy _cut_classes' inequalities); the 3x3 inverse within 1e-9 of the largest
    entry of numpy.linalg.inv (the bound the GPU tests hold these matrices to), the identity exactly, the singular matrix refused; the
    refit within 1e-9 relative of oracle/warp_oracle.py:refit_homography on the masked-in points; the guards at 50 | 51 matches and
    25 | 26 inliers; scratch totals equal to the formula written out here; launch chunks 2, 2, 4, 4, ... summing to ceil(i / 4) + 2."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tvl1_oracle as tv
    import warp_oracle as wo
    import _warp_inputs as wi
    from test_flow_edges_gpu import FIXED, _cut_classes
    from test_warp_oracle import synthetic_matches
    lines, judges = [], []

    def case(text, judge):
        lines.append(text)
        judges.append(judge)

    # pyramid sizes: equal to the oracle's; offsets the running sum times max_pairs
    def pyramid(h, w, ns, step, mp):
        def judge(out):
            v = [int(x) for x in _numbers(out, "pyramid")]
            sizes = tv.pyramid_sizes(h, w, ns, step)
            assert v[0] == len(sizes) and [(a, b) for a, b in zip(v[1::3], v[2::3])] == sizes, (h, w, ns, step, out)
            assert v[3::3] == [mp * int(sum(a * b for a, b in sizes[:k])) for k in range(len(sizes))], out
        case("pyramid %d %d %d %.9g %d" % (h, w, ns, np.float32(step), mp), judge)
    for k, cfg in enumerate(list(dict.fromkeys((c[0], c[1], c[4], c[5]) for c in FIXED)) + [(256, 340, 5, 0.8), (16, 16, 16, 0.95)]):
        pyramid(*cfg, 1 + 7 * k % 5)

    # tile cuts: the recorded ones, which satisfy the inequalities the GPU test names
    with open(os.path.join(ROOT, "tests", "golden", "flow_plan", "tile_cuts.json")) as f:
        recorded = json.load(f)
    slots = recorded["slots"]
    n_cuts = 0
    for shape in recorded["shapes"].values():
        assert len(shape["cuts"]) == 32
        for n, cuts in enumerate(shape["cuts"], 1):
            for (lh, lw), want in zip(shape["levels"], cuts):
                def judge(out, want=want, level=(lh, lw), n=n):
                    got = tuple(int(x) for x in _numbers(out, "tiles"))
                    assert got == tuple(want), (level, n, got, want)
                    _cut_classes(got, level, n, slots)
                case("tiles %d %d %d %d 4 2048" % (lw, lh, n, slots), judge)
                n_cuts += 1
    assert n_cuts == 32 * (3 + 3 + 5 + 5 + 5 + 2 + 1)

    # the 3x3 inverse
    def invert(M, exact=False):
        def judge(out):
            got = np.array(_numbers(out, "invert ok")).reshape(3, 3)
            want = np.linalg.inv(M)
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (M, got, want)
            assert not exact or (got.tobytes() == np.eye(3).tobytes()), got
        case("invert " + " ".join("%.17g" % v for v in M.reshape(-1)), judge)
    for M in (wi.H_MILD, wi.H_PERSPECTIVE, np.linalg.inv(wi.H_PERSPECTIVE), wi.translation_matrix(1, 0), wi.translation_matrix(5, -3), wi.translation_matrix(347, 0)):
        invert(M)
    invert(np.eye(3), exact=True)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    case("invert " + " ".join("%.17g" % v for v in singular.reshape(-1)), lambda out: out == "invert singular" or pytest.fail(out))

    # the refit: only masked-in points count
    def refit(src, dst, mask, expect=True):
        def judge(out):
            if not expect:
                assert out == "refit fail", out
                return
            got = np.array(_numbers(out, "refit ok")).reshape(3, 3)
            want = wo.refit_homography(src[mask], dst[mask])
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (int(mask.sum()), np.abs(got - want).max())
        case("refit %d\n" % len(src) + "\n".join("%.9g %.9g %.9g %.9g %d" % (s[0], s[1], d[0], d[1], m) for s, d, m in zip(src, dst, mask)), judge)
    for n_in in (4, 5, 60, 1000):
        s, d, inl = synthetic_matches(wi.H_PERSPECTIVE, n_in, 0, seed=70 + n_in, noise=0.3)
        refit(s, d, inl)
        s, d, inl = synthetic_matches(wi.H_MILD, n_in, n_in // 2 + 3, seed=80 + n_in, noise=0.3)        # outliers interleaved, masked out
        assert not inl.all() and inl.sum() == n_in
        refit(s, d, inl)
    s, d, inl = synthetic_matches(wi.H_MILD, 3, 20, seed=90, noise=0.3)
    refit(s, d, inl, expect=False)                                                                        # 3 inliers among 23 points
    same = np.full((12, 2), 41.25, np.float32)
    refit(same, same, np.ones(12, bool), expect=False)                                                    # all points coincident

    # the guards of the warped flow
    for matches in (50, 51):
        for inliers in (25, 26):
            keep = matches == 51 and inliers == 26
            def judge(out, keep=keep):
                got = np.array(_numbers(out, "guard kept" if keep else "guard replaced")).reshape(3, 3)
                assert got.tobytes() == (wi.H_PERSPECTIVE if keep else np.eye(3)).tobytes(), out
            case("guard %d %d " % (matches, inliers) + " ".join("%.17g" % v for v in wi.H_PERSPECTIVE.reshape(-1)), judge)
    for matches, inliers in ((51, 1000), (1000, 26)):
        case("guard %d %d " % (matches, inliers) + " ".join("%.17g" % v for v in wi.H_MILD.reshape(-1)),
             lambda out: np.array(_numbers(out, "guard kept")).tobytes() == wi.H_MILD.tobytes() or pytest.fail(out))
    case("guard 1000 1000 " + " ".join("%.17g" % v for v in singular.reshape(-1)),
         lambda out: np.array(_numbers(out, "guard replaced")).tobytes() == np.eye(3).tobytes() or pytest.fail(out))

    # scratch layouts
    for n, most in ((1, 4), (3, 320), (64, 1000), (2, 8192)):
        def judge(out, n=n, most=most):
            h, src, dst, counts, best, winner, mask, total, pts = (int(x) for x in _numbers(out, "ransac_scratch"))
            offs = [h, src, dst, counts, best, winner, mask, total]
            assert offs == sorted(offs) and len(set(offs)) == 8 and h % 8 == 0 and all(o % 4 == 0 for o in (src, dst, counts, best, winner))
            assert (src - h, dst - src, counts - dst, best - counts, winner - best, mask - winner) == (72 * n, pts, pts, 4 * n, 4 * n, 4 * n)
            pts_b = n * most * 2 * 4
            assert pts == pts_b and total == 2 * pts_b + n * (3 * 4 + 9 * 8) + n * most + 64 and total - mask >= n * most
        case("ransac_scratch %d %d" % (n, most), judge)

        def judge_w(out, n=n, most=most):
            corners, moved, counts, total, cb = (int(x) for x in _numbers(out, "warp_scratch"))
            assert (corners, moved, counts) == (0, cb, 2 * cb) and cb == n * most * 2 * 4 and counts % 4 == 0
            assert total == 2 * cb + n * 4
        case("warp_scratch %d %d" % (n, most), judge_w)

    # launch chunks
    for iterations in (1, 4, 5, 300):
        def judge(out, iterations=iterations):
            v = [int(x) for x in _numbers(out, "chunks")]
            most, chunks = v[0], v[1:]
            assert most == -(-iterations // 4) + 2 and sum(chunks) == most
            want = []
            while sum(want) < most:
                want.append(min(2 if sum(want) < 4 else 4, most - sum(want)))
            assert chunks == want, (iterations, chunks)
        case("chunks %d 4" % iterations, judge)

    path = tmp_path / "flow_cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = [ln for ln in _run(drivers["asan"], "flow", str(path)).splitlines() if ln]
    assert len(out) == len(judges), (len(out), len(judges), out[-3:])
    for ln, judge in zip(out, judges):
        judge(ln)
