"""GPU: the ten-crop over-sample on the device -- VQ_RESIZE_OVERSAMPLE / VQ_RESIZE_MIRROR_INVERT on vq_resize_crop and
vq_resize_crop_planes against the pixel loops of tests/_oversample_ref.py, bit for bit (integer and fp64 arithmetic restated operation
for operation: no tolerance), the refusals, FrameIngest.oversample_from_*, the extractors' ``over_sample=True``, CaffeNet(scores=True)
cutting on the device, and ``calcSig_wOF.py --over_sample``.  Order and x-inversion are pyActionRecog's as remembered: parity unpinned."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _oversample_ref as ref
import tsn_oracle as to

pytestmark = pytest.mark.gpu

SOURCES = [(23, 31), (64, 80), (29, 37)]          # (h, w): up-scaling, down-scaling, a frame that has the size of ...
FRAME = (37, 29)                                  # ... the resized frame (w, h)
PLANES_SOURCES = [(23, 31), (64, 80), (30, 38)]
PLANES_FRAME = (38, 30)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev(gpu):
    import torch
    import video_query_algorithms_amd  # noqa: F401
    from video_query_algorithms_amd import _lib
    from video_query_algorithms_amd.tsn import frames

    class Dev:
        pass
    d = Dev()
    d.torch, d.lib, d.frames = torch, _lib, frames
    return d


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _packed_case(src, c, frame_size, crop, rule):
    """Three frames [3][h][w][c] of seeded noise and their ten crops [3][10][crop][crop][c] by the pixel loops (computed once)."""
    x = _noise((3,) + src + (c,), 100 * src[0] + c)
    want = np.stack([ref.ten_crops(f if c > 1 else f[..., 0], frame_size, crop, rule) for f in x])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def _planes_case(src, frame_size, crop, rule):
    """Two flow stacks [2][10][h][w] and their ten crops [2][10][crop][crop][10]."""
    x = _noise((2, 10) + src, 7 * src[0] + crop)
    want = np.stack([ref.ten_crops_flow_stack(list(s), frame_size, crop, rule) for s in x])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def _resize_crop(dev, x, frame_size, crop, rule, n_out_crops, on_device=False, stream=None, dst_channels=None, c0=0, out=None):
    """One vq_resize_crop call on frames x [n][h][w][c] -> the output buffer [n * n_out_crops][crop][crop][dst_channels] (host copy)."""
    torch = dev.torch
    n, h, w, c = x.shape
    dst_channels = dst_channels or c
    if out is None:
        out = torch.full((n * n_out_crops, crop, crop, dst_channels), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
    keep = torch.from_numpy(np.array(x)).cuda() if on_device else np.array(x)
    torch.cuda.synchronize()
    ptr = C.c_void_p(keep.data_ptr()) if on_device else keep.ctypes.data_as(C.c_void_p)
    dev.lib.call("vq_resize_crop", ptr, 1 if on_device else 0, n, h, w, c, frame_size[0], frame_size[1], crop, rule,
                 C.c_void_p(out.data_ptr()), dst_channels, c0, 0, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _resize_crop_planes(dev, stacks, frame_size, crop, rule, n_out_crops):
    """One vq_resize_crop_planes call on stacks [n][10][h][w], handed over plane-major -> [n * n_out_crops][crop][crop][10]."""
    torch = dev.torch
    n, ch, h, w = stacks.shape
    major = torch.from_numpy(np.ascontiguousarray(stacks.transpose(1, 0, 2, 3))).cuda()
    out = torch.full((n * n_out_crops, crop, crop, ch), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev.lib.call("vq_resize_crop_planes", C.c_void_p(major.data_ptr()), n, h, w, ch, n * h * w, frame_size[0], frame_size[1], crop, rule,
                 C.c_void_p(out.data_ptr()), 0, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("rule", ["cv2", "exact"])
@pytest.mark.parametrize("src", SOURCES)
def test_packed_form_against_the_pixel_loops(dev, src, rule):
    """n in {1, 3}, c in {1, 3}, crops 16, 15 (odd) and 18 (3 * 5 * 18 * 18 = 4 860 threads: a partial last block), frames handed over as a
    host and as a device pointer, on a stream of their own."""
    fr = dev.frames
    bits = fr.RESIZE_RULES[rule] | fr.RESIZE_OVERSAMPLE
    stream = dev.torch.cuda.Stream()
    for c in (1, 3):
        for crop in (16, 15, 18):
            x, want = _packed_case(src, c, FRAME, crop, rule)
            for n in (1, 3):
                for on_device in (False, True):
                    got = _resize_crop(dev, x[:n], FRAME, crop, bits, 10, on_device, stream).reshape(n, 10, crop, crop, c)
                    assert (got == want[:n]).all(), (c, crop, n, on_device)
                    assert (got[:, 5:] == got[:, :5, :, ::-1]).all()                        # mirror pairs, whatever the reference says
            plain = _resize_crop(dev, x, FRAME, crop, fr.RESIZE_RULES[rule], 1)
            assert (plain == want[:, 0]).all()                                              # crop 0 has the bytes of the un-flagged call


@pytest.mark.parametrize("rule", ["cv2", "exact"])
@pytest.mark.parametrize("src", [(23, 31), (29, 29)])
def test_five_windows_in_one_place(dev, src, rule):
    """crop 29 on a 29 x 29 resize: every offset is 0, the five crops are one picture and the other five its mirror."""
    fr = dev.frames
    x, want = _packed_case(src, 3, (29, 29), 29, rule)
    got = _resize_crop(dev, x, (29, 29), 29, fr.RESIZE_RULES[rule] | fr.RESIZE_OVERSAMPLE, 10).reshape(3, 10, 29, 29, 3)
    assert (got == want).all()
    assert all((got[:, k] == got[:, 0]).all() and (got[:, 5 + k] == got[:, 0, :, ::-1]).all() for k in range(5))


def test_one_plane_into_a_ten_channel_buffer(dev):
    """dst_channels = 10, dst_channel0 = 3, c = 1 with MIRROR_INVERT: channel 3 of the ten crops, inverted in the mirrors; the other nine
    channels keep the sentinel."""
    fr = dev.frames
    x, _ = _packed_case((23, 31), 1, FRAME, 16, "cv2")
    want = np.stack([ref.ten_crops(f[..., 0], FRAME, 16, "cv2", invert=True) for f in x])
    bits = fr.RESIZE_CV2 | fr.RESIZE_OVERSAMPLE | fr.RESIZE_MIRROR_INVERT
    got = _resize_crop(dev, x, FRAME, 16, bits, 10, dst_channels=10, c0=3).reshape(3, 10, 16, 16, 10)
    assert (got[..., 3:4] == want).all()
    assert (got[:, 5:, :, :, 3] == 255 - got[:, :5, :, ::-1, 3]).all()
    assert (np.delete(got, 3, axis=-1) == SENTINEL).all()


@pytest.mark.parametrize("src,rule", [((23, 31), "cv2"), ((23, 31), "exact"), ((29, 37), "cv2")], ids=["fixed", "exact", "copy"])
def test_one_plane_into_a_ten_channel_buffer_unflagged(dev, src, rule):
    """The un-flagged call of the kernel that also serves the ten-crop cut, c = 1 into dst_channels = 10 at dst_channel0 = 3, n = 3, crop 15
    (675 threads: a partial last block), in its three modes, into a buffer as large as the flagged call's (n * 10 crops): channel 3 of the
    first n crops is crop 0 of the pixel loops and every other byte keeps the sentinel -- the other nine channels, and the crops behind the
    first n, where the mirror store of the flagged instantiation would land (crop row + 5 * crop) if the un-flagged one carried it."""
    fr, torch = dev.frames, dev.torch
    x, want = _packed_case(src, 1, FRAME, 15, rule)
    out = torch.full((30, 15, 15, 10), SENTINEL, dtype=torch.uint8, device="cuda")
    got = _resize_crop(dev, x, FRAME, 15, fr.RESIZE_RULES[rule], 1, dst_channels=10, c0=3, out=out)
    assert got.shape == (30, 15, 15, 10)
    assert (got[:3, ..., 3:4] == want[:, 0]).all()
    assert (np.delete(got[:3], 3, axis=-1) == SENTINEL).all()
    assert (got[3:] == SENTINEL).all()


@pytest.mark.parametrize("rule", ["cv2", "exact"])
@pytest.mark.parametrize("src", PLANES_SOURCES)
def test_planes_form_against_the_pixel_loops_and_the_per_plane_calls(dev, src, rule):
    """n = 2, resized (38, 30), crops 16 and 30 (as high as the frame): fixed point, exact weights and -- source 30 x 38 -- the copy."""
    fr, torch = dev.frames, dev.torch
    bits = fr.RESIZE_RULES[rule] | fr.RESIZE_OVERSAMPLE
    for crop in (16, 30):
        x, want = _planes_case(src, PLANES_FRAME, crop, rule)
        got = _resize_crop_planes(dev, x, PLANES_FRAME, crop, bits, 10).reshape(2, 10, crop, crop, 10)
        assert (got == want).all(), crop
        out = torch.full((20, crop, crop, 10), SENTINEL, dtype=torch.uint8, device="cuda")
        for p in range(10):
            per_plane = _resize_crop(dev, np.ascontiguousarray(x[:, p, :, :, None]), PLANES_FRAME, crop,
                                     bits | (0 if p % 2 else fr.RESIZE_MIRROR_INVERT), 10, on_device=True, dst_channels=10, c0=p, out=out)
        assert (per_plane.reshape(got.shape) == got).all(), crop
        plain = _resize_crop_planes(dev, x, PLANES_FRAME, crop, fr.RESIZE_RULES[rule], 1)
        assert (plain == got[:, 0]).all()


def test_crop0_control(dev):
    """The un-flagged calls (the TEN = false instantiations of the two kernel templates) give crop 0 of the pixel loops."""
    fr = dev.frames
    for rule in ("cv2", "exact"):
        for src in SOURCES:
            x, want = _packed_case(src, 3, FRAME, 16, rule)
            assert (_resize_crop(dev, x, FRAME, 16, fr.RESIZE_RULES[rule], 1) == want[:, 0]).all()
        for src in PLANES_SOURCES:
            x, want = _planes_case(src, PLANES_FRAME, 16, rule)
            assert (_resize_crop_planes(dev, x, PLANES_FRAME, 16, fr.RESIZE_RULES[rule], 1) == want[:, 0]).all()


def test_refusals_launch_nothing(dev):
    """Flag combinations outside the contract fail with the 'unknown resize rule' error (an odd crop of the planes form with its own) and
    leave the output buffer as it was."""
    torch, lib = dev.torch, dev.lib
    x = torch.from_numpy(_noise((2, 23, 31, 1), 1)).cuda()
    stacks = torch.from_numpy(_noise((10, 2, 23, 31), 2)).cuda()
    out = torch.full((20, 16, 16, 10), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def packed(rule, crop=16):
        lib.call("vq_resize_crop", C.c_void_p(x.data_ptr()), 1, 2, 23, 31, 1, 37, 29, crop, rule, C.c_void_p(out.data_ptr()), 10, 0, 0, None)

    def planes(rule, crop=16):
        lib.call("vq_resize_crop_planes", C.c_void_p(stacks.data_ptr()), 2, 23, 31, 10, 2 * 23 * 31, 38, 30, crop, rule, C.c_void_p(out.data_ptr()), 0, None)

    for fn, rule in ((packed, 0x200), (packed, 0x400 | 0x100), (packed, 2 | 0x100), (packed, 0x201), (planes, 0x300), (planes, 0x400 | 0x100),
                     (planes, 2 | 0x100)):
        with pytest.raises(lib.VqError, match="unknown resize rule"):
            fn(rule)
    with pytest.raises(lib.VqError, match="even"):
        planes(0x100, crop=15)
    with pytest.raises(lib.VqError, match="does not fit"):
        packed(0x100, crop=30)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    packed(0x100)                                                    # the good call is accepted
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[..., 0] != SENTINEL).any()


@pytest.mark.parametrize("rule", ["cv2", "exact"])
def test_frame_ingest_at_the_product_size(dev, rule):
    """One 240 x 320 RGB frame and one 10-plane stack -> 340 x 256, crop 224: FrameIngest.oversample_from_frames == frames.oversample*."""
    from video_query_algorithms_amd.tsn.ingest import FrameIngest
    fr = dev.frames
    rgb = _noise((1, 240, 320, 3), 3)
    ing = FrameIngest(3, 0, rule)
    got = ing.oversample_from_frames(rgb)
    ing.sync()
    assert tuple(got.shape) == (10, 224, 224, 3) and (got.cpu().numpy() == fr.oversample(rgb[0], rule=rule)).all()
    ing.close()
    stack = _noise((1, 10, 240, 320), 4)
    ing = FrameIngest(10, 0, rule)
    got = ing.oversample_from_frames(stack)
    ing.sync()
    assert tuple(got.shape) == (10, 224, 224, 10) and (got.cpu().numpy() == fr.oversample_flow_stack(list(stack[0]), rule=rule)).all()
    ing.close()


def test_frame_ingest_from_jpeg_files(dev, tmp_path):
    """Three colour files and two stacks of ten grey files of one size: oversample_from_jpegs == host decode + frames.oversample*, through
    the resize kernels and (frame_size = the files' size) the copy; flow with an even crop (one launch) and an odd one (per plane)."""
    from PIL import Image
    from video_query_algorithms_amd.tsn.ingest import FrameIngest
    fr = dev.frames
    rng = np.random.default_rng(9)
    colour, grey = [], []
    for i in range(3):
        colour.append(str(tmp_path / ("c%d.jpg" % i)))
        Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(colour[-1], quality=90)
    for i in range(20):
        grey.append(str(tmp_path / ("g%d.jpg" % i)))
        Image.fromarray(rng.integers(0, 256, (40, 56), dtype=np.uint8)).save(grey[-1], quality=90)
    ing = FrameIngest(3, 0)
    for frame_size, crop in (((37, 29), 16), ((56, 40), 18)):
        got = ing.oversample_from_jpegs(colour, frame_size, crop).cpu().numpy()
        want = np.concatenate([fr.oversample(fr.imread(f, True), frame_size, crop) for f in colour])
        assert got.shape == (30, crop, crop, 3) and (got == want).all(), frame_size
    ing.close()
    ing = FrameIngest(10, 0)
    for frame_size, crop in (((37, 29), 16), ((37, 29), 15), ((56, 40), 18)):
        got = ing.oversample_from_jpegs(grey, frame_size, crop, lane=1).cpu().numpy()
        want = np.concatenate([fr.oversample_flow_stack([fr.imread(f, False) for f in grey[10 * i:10 * i + 10]], frame_size, crop) for i in range(2)])
        assert got.shape == (20, crop, crop, 10) and (got == want).all(), (frame_size, crop)
    ing.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("c", [3, 10], ids=["rgb", "flow"])
def test_extractors_and_caffenet_cut_on_the_device(dev, c):
    """fc-action, B = 2, T = 2: extract_clips_from_frames(over_sample=True) == TsnNet.forward(host-cut crops, 20, mean), bit for bit (the
    video-level class scores: the fp64 mean over 2 snippets x 10 crops); CaffeNet(scores=True) cutting on the device and with
    host_oversample=True return the same bits."""
    from video_query_algorithms_amd.tsn import bn_inception as bi, caffe_net, net
    fr = dev.frames
    g = bi.bn_inception(c)
    w = net.synthetic_weights(g, seed=2 if c == 3 else 5)
    mean = net.RGB_MEAN if c == 3 else net.FLOW_MEAN
    if c == 3:
        x = _noise((4, 240, 320, 3), 31)
        host = np.concatenate([fr.oversample(f) for f in x])
    else:
        x = _noise((4, 10, 240, 320), 32)
        host = np.concatenate([fr.oversample_flow_stack(list(s)) for s in x])
    cn = caffe_net.CaffeNet(g, w, 0, max_crops=40, feature_blob="fc-action")
    try:
        got = cn.extract_clips_from_frames(x, 2, over_sample=True)
        want, ps = cn._model.forward(host, 20, mean)
        assert got.shape == (2, 101) and got.dtype == np.float64 and (_bits(got) == _bits(want)).all()
        assert (want == to.consensus(ps, 20)).all()
        crops = cn.oversample_from_frames(x)
        cn.sync_ingest()
        assert (_bits(cn.extract_clips_from_crops(crops, 2, over_sample=True)) == _bits(want)).all()
        on_dev = cn.extract_clips_from_frames(x, 2, on_device=True, over_sample=True)
        assert on_dev.is_cuda and (_bits(on_dev.cpu().numpy()) == _bits(want)).all()
    finally:
        cn.close()
    small = caffe_net.CaffeNet(g, w, 0, max_crops=19, feature_blob="fc-action")
    try:
        with pytest.raises(ValueError):
            small.extract_clips_from_frames(x, 2, over_sample=True)              # 19 < 10 T
    finally:
        small.close()
    on_device = caffe_net.CaffeNet(g, w, 0, max_crops=2, scores=True)
    on_host = caffe_net.CaffeNet(g, w, 0, max_crops=2, scores=True, host_oversample=True)
    try:
        frame = [x[0]] if c == 3 else list(x[0])
        call = (lambda o: o.predict_single_frame(frame, "fc-action")) if c == 3 else (lambda o: o.predict_single_flow_stack(frame, "fc-action"))
        a, b = call(on_device), call(on_host)
        assert a.shape == (10, 101) and a.dtype == np.float32 and (_bits(a) == _bits(b)).all()
        for blob in ("global_pool", "fc-action"):
            assert on_device._net.blobs[blob].data.tobytes() == on_host._net.blobs[blob].data.tobytes()
    finally:
        on_device.close()
        on_host.close()


def test_command_line_over_sample(dev, tmp_path):
    """``--over_sample --featureBlob fc-action --featureBlob_size 101`` on two clips of JPEG frames (one of 340 x 256: the copy; one of
    320 x 240: the resize), T = 3, host-decoded and with ``--device_jpeg``: the rows of both streams are the reprs of ``extract_clips`` on
    host-cut crops with T' = 30."""
    from PIL import Image
    from video_query_algorithms_amd import calcSig_wOF
    from video_query_algorithms_amd.tsn import bn_inception as bi, caffe_net, net
    import test_tsn_gpu as base
    fr = dev.frames
    rng = np.random.default_rng(29)
    root = tmp_path / "frames"
    clips = {"clip_0001": (6, (256, 340)), "clip_0002": (7, (240, 320))}
    for clip, (n, hw) in clips.items():
        d = root / "va" / clip
        d.mkdir(parents=True)
        for i in range(1, n + 1):
            Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(str(d / ("img_%05d.jpg" % i)), quality=90)
            for axis in "xy":
                Image.fromarray(rng.integers(0, 256, hw, dtype=np.uint8)).save(str(d / ("flow_%s_%05d.jpg" % (axis, i))), quality=90)
    protos = base._write_protos(bi, tmp_path)
    wfile, weights = {}, {}
    for name, c, seed in (("rgb", 3, 2), ("flow", 10, 5)):
        weights[name] = net.synthetic_weights(bi.bn_inception(c), seed=seed)
        wfile[name] = str(tmp_path / ("ucf101_split1_tsn_%s_bn.npz" % name))
        caffe_net.save_weights(wfile[name], weights[name])

    def run(out, *extra):
        return calcSig_wOF.main([str(root), protos["rgb"], wfile["rgb"], protos["flow"], wfile["flow"], "--num_frame_per_video", "3",
                                 "--outFeatures_dir", str(out), "--modelname", "UCF101_split1", "--batch_clips", "2", "--num_worker", "2",
                                 "--over_sample", "--featureBlob", "fc-action", "--featureBlob_size", "101"] + list(extra))

    def tree(out):
        found = {}
        for dirpath, _, files in os.walk(str(out)):
            for fn in files:
                with open(os.path.join(dirpath, fn), "rb") as f:
                    found[os.path.relpath(os.path.join(dirpath, fn), str(out))] = f.read()
        return found

    assert run(tmp_path / "host") == 0
    assert run(tmp_path / "dev", "--device_jpeg") == 0
    host, device = tree(tmp_path / "host"), tree(tmp_path / "dev")
    assert len(host) == 2 and host == device                                     # one video x two streams, identical bytes
    for name, c, mean, mode in (("rgb", 3, net.RGB_MEAN, "rgb"), ("flow", 10, net.FLOW_MEAN, "warped_optical_flow")):
        cn = caffe_net.CaffeNet(bi.bn_inception(c), weights[name], 0, max_crops=30, feature_blob="fc-action")
        try:
            path = [p for p in host if mode in os.path.basename(p)]
            assert len(path) == 1
            rows = [l.split(",") for l in host[path[0]].decode().splitlines() if l and l[0].isdigit()]
            assert [int(r[0]) for r in rows] == [1, 2]
            for r, (clip, (n, _)) in zip(rows, clips.items()):
                d = str(root / "va" / clip)
                ticks = to.frame_ticks(n, 3, 1 if c == 3 else 5)
                crops = fr.load_rgb_oversampled(d, ticks) if c == 3 else fr.load_flow_oversampled(d, ticks, n)
                feat = cn.extract_clips(crops, 30)
                assert len(r) == 102 and r[1:] == [repr(float(v)) for v in feat[0]]
        finally:
            cn.close()
