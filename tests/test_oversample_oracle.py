"""CPU: the ten-crop over-sample of tsn/frames.py (what ``--host_resize --over_sample`` cuts, and what the device kernels are held to
through tests/_oversample_ref.py) against the pixel-loop restatement; the comparison notices four injected errors; the flag values of
the C header and of tsn/frames.py agree; the command line knows ``--over_sample``."""
import os
import re

import numpy as np
import pytest

import _oversample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source h, source w), frame_size (w, h), crop: up-scaling, down-scaling, a frame that has the size; all five windows in one place
CASES = [((23, 31), (37, 29), 16), ((64, 80), (37, 29), 16), ((29, 37), (37, 29), 16), ((23, 31), (29, 29), 29), ((29, 29), (29, 29), 29)]


def _frames():
    import video_query_algorithms_amd  # noqa: F401
    from video_query_algorithms_amd.tsn import frames
    return frames


def _noise(shape, seed):
    """Seeded noise with no symmetry: a mirrored or transposed window cannot pass for the right one."""
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("rule", ["cv2", "exact"])
@pytest.mark.parametrize("src,frame_size,crop", CASES)
def test_host_oversample_equals_the_pixel_loops(src, frame_size, crop, rule):
    frames = _frames()
    rgb = _noise(src + (3,), 11)
    got = frames.oversample(rgb, frame_size, crop, rule)
    assert got.shape == (10, crop, crop, 3) and got.dtype == np.uint8
    assert (got == ref.ten_crops(rgb, frame_size, crop, rule)).all()
    grey = _noise(src, 12)
    assert (frames.oversample(grey, frame_size, crop, rule) == ref.ten_crops(grey, frame_size, crop, rule)).all()
    stack = [_noise(src, 20 + p) for p in range(10)]
    got = frames.oversample_flow_stack(stack, frame_size, crop, rule)
    assert got.shape == (10, crop, crop, 10)
    assert (got == ref.ten_crops_flow_stack(stack, frame_size, crop, rule)).all()
    assert (got[0] == np.stack([frames.crop0(p, frame_size, crop, rule) for p in stack], axis=-1)).all()      # crop 0 is crop0


def test_window_offsets_are_the_python_helpers():
    frames = _frames()
    for h, w, c in ((29, 37, 16), (29, 37, 15), (30, 38, 16), (29, 29, 29), (256, 340, 224), (30, 38, 30)):
        assert ref.windows(h, w, c) == frames.oversample_offsets(h, w, c)


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_the_comparison_notices_an_injected_error(fault):
    frames = _frames()
    src, frame_size, crop = (23, 31), (37, 29), 16
    stack = [_noise(src, 20 + p) for p in range(10)]
    good = frames.oversample_flow_stack(stack, frame_size, crop)
    assert (good == ref.ten_crops_flow_stack(stack, frame_size, crop)).all()
    assert not (good == ref.ten_crops_flow_stack(stack, frame_size, crop, fault=fault)).all()
    if fault != "no_invert":                                    # the RGB form has no inverted plane
        rgb = _noise(src + (3,), 11)
        assert not (frames.oversample(rgb, frame_size, crop) == ref.ten_crops(rgb, frame_size, crop, fault=fault)).all()


def test_flag_values_are_the_headers():
    frames = _frames()
    with open(os.path.join(ROOT, "include", "vq_amd.h")) as f:
        header = f.read()
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(VQ_RESIZE_\w+)\s+(\w+)\s*$", header, flags=re.M)}
    assert defines["VQ_RESIZE_OVERSAMPLE"] == frames.RESIZE_OVERSAMPLE == 0x100
    assert defines["VQ_RESIZE_MIRROR_INVERT"] == frames.RESIZE_MIRROR_INVERT == 0x200
    assert defines["VQ_RESIZE_CV2_FIXED"] == frames.RESIZE_CV2 and defines["VQ_RESIZE_EXACT"] == frames.RESIZE_EXACT
    assert all(v < 0x100 for v in frames.RESIZE_RULES.values())                    # the rule stays in the low byte


def test_command_line_knows_over_sample():
    import video_query_algorithms_amd  # noqa: F401
    from video_query_algorithms_amd import calcSig_wOF
    base = ["frames", "a.prototxt", "a.npz", "b.prototxt", "b.npz"]
    assert calcSig_wOF.build_parser().parse_args(base).over_sample is False
    assert calcSig_wOF.build_parser().parse_args(base + ["--over_sample"]).over_sample is True


def test_command_line_host_oversample_batches_ten_crops_per_snippet(tmp_path):
    """``--over_sample --host_resize`` with the stand-in extractor: every forward gets whole clips of 10 T crops, at most
    max(batch_clips T, 10 T) of them, and a clip's row is the stand-in's function of ``frames.load_*_oversampled``."""
    frames = _frames()
    from video_query_algorithms_amd import calcSig_wOF
    from video_query_algorithms_amd.tsn import feature_csv
    import _cli_standin as cs
    rng = np.random.default_rng(5)
    counts = {"clip_0001": 6, "clip_0002": 7, "clip_0003": 6}
    for clip, n in counts.items():
        d = tmp_path / "frames" / "vid" / clip
        d.mkdir(parents=True)
        for i in range(1, n + 1):
            frames.write_pnm(str(d / ("img_%05d.ppm" % i)), rng.integers(0, 256, (256, 340, 3), dtype=np.uint8))
            for axis in "xy":
                frames.write_pnm(str(d / ("flow_%s_%05d.ppm" % (axis, i))), rng.integers(0, 256, (240, 320), dtype=np.uint8))
    seen = []

    class Net(cs.StandInNet):
        def extract_clips(self, crops, T, on_device=False):
            seen.append((crops.shape[0], T, self.max_crops))
            return super().extract_clips(crops, T, on_device)

    for batch_clips, clips_per_forward in ((2, 1), (25, 2)):             # 2 * 2 < 10 * 2: raised to one clip; 25 * 2 // 20 = 2 clips
        del seen[:]
        out = tmp_path / ("out%d" % batch_clips)
        rc = calcSig_wOF.main([str(tmp_path / "frames"), "r.prototxt", "r_weights.npz", "f.prototxt", "f_weights.npz", "--num_frame_per_video", "2",
                               "--outFeatures_dir", str(out), "--modelname", "M_split1", "--frame_ext", ".ppm", "--batch_clips", str(batch_clips),
                               "--host_resize", "--over_sample"], net_factory=Net)
        assert rc == 0
        want_max = max(batch_clips * 2, 20)
        assert seen and all(T == 20 and n % 20 == 0 and n <= clips_per_forward * 20 and mc == want_max for n, T, mc in seen)
        assert max(n for n, _, _ in seen) == clips_per_forward * 20
        _, streams = feature_csv.read_split_dir(str(out / "vid" / "M_split1"))
        for mode, weights in (("rgb", "r_weights.npz"), ("warped_optical_flow", "f_weights.npz")):
            clips, feats, _ = streams[mode]
            assert clips.tolist() == [1, 2, 3]
            net = cs.StandInNet(None, weights)
            for row, (clip, n) in zip(feats, counts.items()):
                d = str(tmp_path / "frames" / "vid" / clip)
                if mode == "rgb":
                    crops = frames.load_rgb_oversampled(d, frames.frame_ticks(n, 2, 1), ext=".ppm")
                else:
                    crops = frames.load_flow_oversampled(d, frames.frame_ticks(n, 2, 5), n, ext=".ppm")
                assert crops.shape[0] == 20 and (row == net._clip_feature(crops)).all()
