"""GPU: the TV-L1 kernels (csrc/vq_flow.hip through the C ABI) against oracle/tvl1_oracle.py on the same frames.

PARITY UNPINNED with respect to the reference: its flow comes from the third-party ``extract_warp_gpu -b 20 -t 1 -s 1``
(build_wof_clips.py:70-73), absent from the tree together with any frame or flow image.  The oracle restates the
published algorithm; the kernels follow it operation for operation in fp32.  Tolerance: with a fixed number of inner
iterations (epsilon = 0) the fields agree to 1e-4 px (observed ~1e-6: only the rounding of sqrt / division and the fp64
error sum can differ); with the convergence test active a pair may stop one iteration apart when its error grazes the
threshold, so the fields are compared at 2e-2 px and the 8-bit images may differ by one grey level on < 0.5 % of the pixels."""
import numpy as np
import pytest

import tvl1_oracle as tv
from test_flow_oracle import _shifted_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def flow_mod(gpu):
    from video_query_algorithms_amd.tsn import flow
    return flow


def test_fixed_iteration_count_matches_the_oracle_to_rounding(flow_mod):
    pairs = [_shifted_pair(64, 80, 2.5, -1.0, seed=1), _shifted_pair(64, 80, -1.25, 0.5, seed=2), _shifted_pair(64, 80, 0.0, 0.0, seed=3)]
    f0, f1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    m = flow_mod.Tvl1Flow(4, 64, 80, epsilon=0.0, iterations=20, warps=3, nscales=3)
    assert m.levels == tv.pyramid_sizes(64, 80, 3)
    r = m.flow(f0, f1, iterations=True)
    assert (r["iters"][:, :, :2] == 20).all() and (r["iters"][:, :, 2] == 1).all()    # identical frames: the first update is exactly 0
    for i in range(3):
        u1, u2, _ = tv.tvl1_flow(f0[i], f1[i], nscales=3, warps=3, iterations=20, epsilon=0.0)
        assert np.abs(r["u1"][i] - u1).max() <= 1e-4 and np.abs(r["u2"][i] - u2).max() <= 1e-4
        assert (r["flow_x"][i] == tv.flow_to_image(r["u1"][i])).all() and (r["flow_y"][i] == tv.flow_to_image(r["u2"][i])).all()
    assert (r["u1"][2] == 0).all() and (r["u2"][2] == 0).all()
    m.close()


def test_default_parameters_batch_against_the_oracle(flow_mod):
    """OpenCV's defaults (5 scales, 5 warps, epsilon 0.01, up to 300 iterations) on a batch of 340 x 256 pairs with
    different motions: per-pair convergence on the device, fields and 8-bit images against the oracle, motion recovered."""
    motions = [(3.0, -1.5), (-6.5, 2.0), (0.4, 0.3), (4.0, -3.0)]
    pairs = [_shifted_pair(256, 340, dx, dy, seed=10 + k, margin=40) for k, (dx, dy) in enumerate(motions)]
    f0, f1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    m = flow_mod.Tvl1Flow(8, 256, 340)
    r = m.flow(f0, f1, iterations=True)
    assert r["iters"].shape == (5, 5, 4) and r["iters"].min() >= 1 and r["iters"].max() <= 300
    inner = (slice(24, -24), slice(24, -24))
    for i, (dx, dy) in enumerate(motions):
        u1, u2, counts = tv.tvl1_flow(f0[i], f1[i])
        assert abs(np.median(r["u1"][i][inner]) - dx) < 0.15 and abs(np.median(r["u2"][i][inner]) - dy) < 0.15
        assert np.abs(r["u1"][i] - u1).max() <= 2e-2 and np.abs(r["u2"][i] - u2).max() <= 2e-2
        assert np.abs(r["iters"][:, :, i] - np.array(counts)).max() <= 1
        for got, want in ((r["flow_x"][i], tv.flow_to_image(u1)), (r["flow_y"][i], tv.flow_to_image(u2))):
            d = np.abs(got.astype(int) - want.astype(int))
            assert d.max() <= 1 and (d > 0).mean() < 0.005
    # the same pairs one at a time: a pair's result does not depend on its batch
    solo = m.flow(f0[1:2], f1[1:2])
    assert (solo["u1"][0] == r["u1"][1]).all() and (solo["flow_y"][0] == r["flow_y"][1]).all()
    m.close()


def test_homography_warp_and_consecutive_frames(flow_mod):
    """A known camera translation handed over as a homography is compensated before the flow is computed (the matrix
    itself comes from SURF + RANSAC in the reference's binary: not built); consecutive() chains frames like -s 1."""
    f0, f1 = _shifted_pair(96, 128, 4.0, 0.0, seed=5, margin=32)
    m = flow_mod.Tvl1Flow(4, 96, 128)
    h = np.array([[1, 0, -4.0], [0, 1, 0], [0, 0, 1]])              # moves frame1's content back by 4 px
    r = m.flow(f0[None], f1[None], homographies=h[None])
    want1 = tv.warp_homography(f1, h)
    u1, u2, _ = tv.tvl1_flow(f0, want1)
    inner = (slice(16, -16), slice(16, -16))
    assert abs(np.median(r["u1"][0][inner])) < 0.15
    assert np.abs(r["u1"][0] - u1).max() <= 2e-2 and np.abs(r["u2"][0] - u2).max() <= 2e-2
    frames = np.stack([_shifted_pair(96, 128, 1.5 * k, 0.0, seed=5, margin=32)[1] for k in range(4)])
    fx, fy = m.consecutive(frames)
    assert fx.shape == (3, 96, 128) and fx.dtype == np.uint8
    assert abs(np.median(fx[:, 16:-16, 16:-16]) - tv.flow_to_image(np.array([1.5]))[0]) <= 1 and abs(int(np.median(fy)) - 128) <= 1
    with pytest.raises(Exception):
        m.flow(f0[None, :50], f1[None, :50])
    m.close()


def test_blocked_tiles_against_the_oracle_on_every_cut(flow_mod):
    """The inner loop runs in blocks of 4 iterations per launch on tiles FITTED to the level (the fields of a tile resident in
    registers / LDS with a 4-pixel halo, the two sets of planes ping-ponging, the stopping rule kept exact by replaying a block that
    ran past the stop).  With a fixed iteration count (epsilon = 0) the kernel follows the oracle operation for operation: 1e-4 px
    (observed ~1e-6) on shapes that exercise the cut -- iteration counts that are and are not multiples of the block (the tail block
    runs fewer), frames smaller than a tile and larger than several, a single row / column of tiles, tiles wider than 64 cells -- and
    the cut itself (it depends on the level AND on the number of pairs in the batch) never changes a bit: a pair gives the same fields
    alone, in its batch and in a batch whose number of pairs is CHOSEN (Tvl1Flow.tile_cuts) for a cut that differs from its batch's on at
    least one level -- for these frames most small pair counts share one cut.  (Rounds 2-4 also kept the un-blocked two-launch form and
    the square-tile form in the library and compared them with this kernel bit for bit; they were removed in round 5.)"""
    rng = np.random.default_rng(31)
    for (h, w, iters, warps, scales, n) in ((64, 80, 7, 2, 3, 3), (100, 132, 12, 3, 2, 1), (256, 340, 6, 1, 5, 9), (48, 50, 9, 2, 2, 2), (40, 300, 5, 1, 1, 3),
                                            (131, 174, 8, 1, 1, 4)):
        pairs = [_shifted_pair(h, w, float(rng.uniform(-3, 3)), float(rng.uniform(-2, 2)), seed=300 + k, margin=12) for k in range(n)]
        f0, f1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        m = flow_mod.Tvl1Flow(n, h, w, epsilon=0.0, iterations=iters, warps=warps, nscales=scales)
        r = m.flow(f0, f1, iterations=True)
        assert (r["iters"] == iters).all()
        for i in (0, n - 1):
            u1, u2, _ = tv.tvl1_flow(f0[i], f1[i], nscales=scales, warps=warps, iterations=iters, epsilon=0.0)
            assert np.abs(r["u1"][i] - u1).max() <= 1e-4 and np.abs(r["u2"][i] - u2).max() <= 1e-4, (h, w, i)
        solo = m.flow(f0[n - 1:], f1[n - 1:])                       # another number of pairs; whether it is another cut depends on the level sizes
        assert (solo["u1"][0] == r["u1"][n - 1]).all() and (solo["u2"][0] == r["u2"][n - 1]).all(), (h, w)
        m.close()
        big = flow_mod.Tvl1Flow(32, h, w, epsilon=0.0, iterations=iters, warps=warps, nscales=scales)
        other = next(k for k in range(1, 33) if big.tile_cuts(k) != big.tile_cuts(n))      # ... this one IS another cut of at least one level
        order = [q % n for q in range(other - 1)] + [n - 1]          # the same pair last, the others before it
        many = big.flow(f0[order], f1[order])
        assert (many["u1"][-1] == r["u1"][n - 1]).all() and (many["u2"][-1] == r["u2"][n - 1]).all(), (h, w, other)
        big.close()
    # identical frames stop after exactly one iteration (the first block is replayed with one iteration)
    f = _shifted_pair(96, 128, 0.0, 0.0, seed=7)[0]
    m = flow_mod.Tvl1Flow(2, 96, 128)
    r = m.flow(f[None], f[None], iterations=True)
    assert (r["iters"] == 1).all() and (r["u1"] == 0).all() and (r["u2"] == 0).all()
    m.close()


def test_packed_division_and_square_root_are_the_compilers_bit_for_bit(tmp_path):
    """csrc/vq_flow_math.h writes the correctly rounded division and square root out (so that their refinement runs as packed instructions on
    two cells at a time); tools/ubench/flow_math_check.hip compares them with `a / b` and sqrtf() on 2^24 x 2 operand pairs per case --
    raw bit patterns (denormals, zeros, infinities, NaNs), the dual step's ranges, numerators that are exact zeros, sums of squares down
    to the library's scaled path.  Compiled here with the flags of the library."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "flow_math_check")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(root, "video-query-algorithms_amd", "csrc"),
                    os.path.join(root, "tools", "ubench", "flow_math_check.hip"), "-o", exe], check=True, capture_output=True, timeout=300)
    p = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.count(" 0 mismatches") == 5
