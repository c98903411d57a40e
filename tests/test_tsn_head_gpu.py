"""GPU: the fc-action head (VQ_OP_INNER_PRODUCT) in isolation, its batch invariance, both whole networks with the head, the
descriptions vq_tsn_create must refuse, and the command line with ``--featureBlob fc-action``.

Tolerances (the project's): one layer |d| <= 2e-5 max|y| against fp64 on the device's own input; a whole network
|d| <= 2e-4 max|y| against the fp64 oracle's global_pool pushed through the fp64 head (tests/_tsn_head.py); consensus bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import _tsn_head as th
import tsn_oracle as to

pytestmark = pytest.mark.gpu

HEAD_CASES = [(1024, 101), (96, 1), (40, 130), (64, 64)]      # N not a multiple of 4 / 32, K not a multiple of 64 / 256
HEAD_CROPS = [1, 3, 7, 33]                                    # less than a 4-row wave, ragged, more than 32 rows


@pytest.fixture(scope="module")
def tsn(gpu):
    import video_query_algorithms_amd  # noqa: F401
    from video_query_algorithms_amd.tsn import bn_inception, net
    return bn_inception, net


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("k,n", HEAD_CASES)
def test_head_in_isolation(tsn, k, n):
    bi, net = tsn
    g = th.head_graph(bi, k, n)
    w = net.synthetic_weights(g, seed=k + n)
    m = net.TsnNet(g, w, max_crops=max(HEAD_CROPS), feature_blob="fc")
    try:
        assert m.feature_dim == n and m.layer_op(len(m.plan.ops) - 1) == 7
        for crops_n in HEAD_CROPS:
            crops = np.random.default_rng(crops_n).integers(0, 256, (crops_n, 4, 4, 32), dtype=np.uint8)
            feat, ps = m.forward(crops, 1, [128.0] * 32)
            gp = m.read_blob("gp", crops_n).reshape(crops_n, k)
            want = th.head_fp64(w["fc"]["W"], w["fc"]["b"], gp)
            err = np.abs(ps - want).max() / np.abs(want).max()
            print("K=%d N=%d crops=%d: max|d|/max|y| = %.2e" % (k, n, crops_n, err))
            assert ps.shape == (crops_n, n) and err <= 2e-5
            assert (feat == ps.astype(np.float64)).all()                       # T = 1: the consensus is the score itself
            assert (m.read_blob("fc", crops_n).reshape(crops_n, n) == ps).all()
        tiles = m.layer_tiles(HEAD_CROPS[-1])
        assert (tiles[-1] == 0).all()                                          # no tiling choices
    finally:
        m.close()


@pytest.mark.parametrize("split", ["1", "2", "3", "2,1"])
def test_head_scores_do_not_depend_on_the_batch(tsn, monkeypatch, split):
    """Crop i of a 33-crop forward, alone, at other positions of a 6-crop batch, under every sub-batch split: the same bits."""
    bi, net = tsn
    g = th.head_graph(bi, 1024, 101)
    w = net.synthetic_weights(g, seed=4)
    crops = np.random.default_rng(2).integers(0, 256, (33, 4, 4, 32), dtype=np.uint8)
    mean = [128.0] * 32
    monkeypatch.setenv("VQ_TSN_SPLIT", "1")
    m = net.TsnNet(g, w, max_crops=33, feature_blob="fc")
    base = m.forward(crops, 1, mean)[1]
    m.close()
    monkeypatch.setenv("VQ_TSN_SPLIT", split)
    m = net.TsnNet(g, w, max_crops=33, feature_blob="fc")
    try:
        for i in (0, 17, 32):
            alone = m.forward(crops[i:i + 1], 1, mean)[1]
            assert (_bits(alone[0]) == _bits(base[i])).all()
            order = [i, 1, 2, 30, 31, i]                                       # 6 crops: every split of the list divides them
            six = m.forward(crops[order], 3, mean)[1]
            assert (_bits(six) == _bits(base[order])).all()
        assert (_bits(m.forward(crops, 1, mean)[1]) == _bits(base)).all()      # 33 crops: "3" cuts 11 + 11 + 11, "2,1" 22 + 11
    finally:
        m.close()


@pytest.mark.parametrize("c", [3, 10], ids=["rgb", "flow"])
def test_whole_network_with_the_head(tsn, c):
    bi, net = tsn
    g = bi.bn_inception(c)
    w = net.synthetic_weights(g, seed=2 if c == 3 else 5)
    mean = net.RGB_MEAN if c == 3 else net.FLOW_MEAN
    crops = np.random.default_rng(30 + c).integers(0, 256, (6, 224, 224, c), dtype=np.uint8)
    m = net.TsnNet(g, w, max_crops=6, feature_blob="fc-action")
    plain = net.TsnNet(g, w, max_crops=6)
    try:
        assert m.feature_dim == 101 and m.graph_key != plain.graph_key           # the two plans never share a tiling table
        assert m.flops_per_crop() == plain.flops_per_crop() + 2.0 * 1024 * 101
        feat, ps = m.forward(crops, 3, mean)
        gp_feat, gp_ps = plain.forward(crops, 3, mean)
        gp = m.read_blob("global_pool", 6).reshape(6, 1024)
        assert (_bits(gp) == _bits(gp_ps)).all()                                 # the interior global pool: the bits of the default net
        ref_gp = to.forward(g.layers, "data", w, to.preprocess(crops, mean), keep=("global_pool",))["global_pool"].reshape(6, -1)
        want = th.head_fp64(w["fc-action"]["W"], w["fc-action"]["b"], ref_gp)
        err = np.abs(ps - want).max() / np.abs(want).max()
        print("%s: scores max|d|/max|y| = %.2e, %d of %d negative" % ("rgb" if c == 3 else "flow", err, (ps < 0).sum(), ps.size))
        assert ps.shape == (6, 101) and err <= 2e-4
        assert (ps < 0).any() and (ps > 0).any()
        assert (feat == to.consensus(ps, 3)).all() and feat.shape == (2, 101)
        # keep=: the default features AND the scores from one forward
        both = net.TsnNet(g, w, max_crops=6, keep=("fc-action",))
        try:
            f2, p2 = both.forward(crops, 3, mean)
            assert (f2 == gp_feat).all() and (_bits(p2) == _bits(gp_ps)).all()
            assert (_bits(both.read_blob("fc-action", 6).reshape(6, 101)) == _bits(ps)).all()
        finally:
            both.close()
    finally:
        m.close()
        plain.close()


def test_bad_inner_product_descriptions_are_refused(tsn):
    """vq_tsn_create validates VQ_OP_INNER_PRODUCT before anything is launched: 1x1 slots, channels within them, offsets in the blob."""
    from video_query_algorithms_amd import _lib
    tensors = (_lib.TensorDesc * 3)(_lib.TensorDesc(4, 4, 32), _lib.TensorDesc(1, 1, 32), _lib.TensorDesc(1, 1, 5))
    blob = np.zeros(32 * 5 + 8, dtype=np.float32)
    inp = _lib.InputDesc(4, 4, 32, -1, 0, 0)
    segs = (_lib.ConvSegment * 1)()

    def create(**change):
        fc = dict(op=_lib.VQ_OP_INNER_PRODUCT, src=1, dst=2, src_coff=0, dst_coff=0, cin=32, cout=5, k=1, stride=1, pad=0, relu=0, ceil_mode=1,
                  has_bias=1, seg_first=0, seg_count=0, pre_pool_k=0, pre_pool_stride=0, w_off=0, b_off=160)
        fc.update(change)
        layers = (_lib.LayerDesc * 2)(
            _lib.LayerDesc(op=_lib.VQ_OP_GLOBAL_AVGPOOL, src=0, dst=1, src_coff=0, dst_coff=0, cin=32, cout=32, k=4, stride=1, pad=0, relu=0,
                           ceil_mode=1, has_bias=0, seg_first=0, seg_count=0, pre_pool_k=0, pre_pool_stride=0, w_off=0, b_off=0),
            _lib.LayerDesc(**fc))
        h = C.c_void_p()
        try:
            _lib.call("vq_tsn_create", tensors, 3, layers, 2, segs, 0, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(inp), 2, 2, 0, C.byref(h))
        finally:
            if h:
                _lib.load().vq_tsn_destroy(h)

    create()                                                   # the good description is accepted
    for change in (dict(src=0, cin=32), dict(cout=6), dict(dst_coff=1), dict(cin=36), dict(cin=30), dict(src_coff=2), dict(w_off=12),
                   dict(w_off=2), dict(b_off=164), dict(b_off=-1), dict(relu=1), dict(has_bias=0)):
        with pytest.raises(_lib.VqError):
            create(**change)


def test_command_line_writes_class_scores(tsn, tmp_path):
    """``--featureBlob fc-action --featureBlob_size 101`` on two videos x two clips of 340 x 256 JPEGs, host-decoded and with
    ``--device_jpeg``: the same bytes, 101 signed columns, every token the repr of the consensus computed through the Python objects;
    a wrong ``--featureBlob_size`` fails."""
    bi, net = tsn
    from PIL import Image
    from video_query_algorithms_amd import calcSig_wOF
    from video_query_algorithms_amd.tsn import caffe_net, frames
    import test_tsn_gpu as base
    rng = np.random.default_rng(23)
    root = tmp_path / "frames"
    counts = {("va", "clip_0001"): 6, ("va", "clip_0002"): 7, ("vb", "clip_0001"): 8, ("vb", "clip_0003"): 6}
    for (video, clip), n in counts.items():
        d = root / video / clip
        d.mkdir(parents=True)
        for i in range(1, n + 1):
            Image.fromarray(rng.integers(0, 256, (256, 340, 3), dtype=np.uint8)).save(str(d / ("img_%05d.jpg" % i)), quality=90)
            for axis in "xy":
                Image.fromarray(rng.integers(0, 256, (256, 340), dtype=np.uint8)).save(str(d / ("flow_%s_%05d.jpg" % (axis, i))), quality=90)
    protos = base._write_protos(bi, tmp_path)
    wfile, weights = {}, {}
    for name, c, seed in (("rgb", 3, 2), ("flow", 10, 5)):
        weights[name] = net.synthetic_weights(bi.bn_inception(c), seed=seed)
        wfile[name] = str(tmp_path / ("ucf101_split1_tsn_%s_bn.npz" % name))
        caffe_net.save_weights(wfile[name], weights[name])

    def run(out, *extra):
        return calcSig_wOF.main([str(root), protos["rgb"], wfile["rgb"], protos["flow"], wfile["flow"], "--num_frame_per_video", "3",
                                 "--outFeatures_dir", str(out), "--modelname", "UCF101_split1", "--batch_clips", "2", "--num_worker", "2",
                                 "--featureBlob", "fc-action"] + list(extra))

    def tree(out):
        found = {}
        for dirpath, _, files in os.walk(str(out)):
            for fn in files:
                with open(os.path.join(dirpath, fn), "rb") as f:
                    found[os.path.relpath(os.path.join(dirpath, fn), str(out))] = f.read()
        return found

    assert run(tmp_path / "host", "--featureBlob_size", "101") == 0
    assert run(tmp_path / "dev", "--featureBlob_size", "101", "--device_jpeg") == 0
    host, dev = tree(tmp_path / "host"), tree(tmp_path / "dev")
    assert len(host) == 4 and host == dev                                        # two videos x two streams, identical bytes
    negative = 0
    for name, c, mean, mode in (("rgb", 3, net.RGB_MEAN, "rgb"), ("flow", 10, net.FLOW_MEAN, "warped_optical_flow")):
        m = net.TsnNet(bi.bn_inception(c), weights[name], max_crops=3, feature_blob="fc-action")
        try:
            for video in ("va", "vb"):
                path = [p for p in host if p.startswith(video + os.sep) and mode in os.path.basename(p)]
                assert len(path) == 1 and "fc-action" in os.path.basename(path[0])
                lines = host[path[0]].decode().splitlines()
                assert "feature blob =fc-action" in "\n".join(lines[:12])
                rows = [l.split(",") for l in lines if l and l[0].isdigit()]
                clips = sorted(k[1] for k in counts if k[0] == video)
                assert [int(r[0]) for r in rows] == [int(cl.split("_")[1]) for cl in clips]
                for r, clip in zip(rows, clips):
                    n = counts[(video, clip)]
                    d = str(root / video / clip)
                    ticks = to.frame_ticks(n, 3, 1 if c == 3 else 5)
                    crops = frames.load_rgb_snippets(d, ticks) if c == 3 else frames.load_flow_snippets(d, ticks, n)
                    feat, _ = m.forward(crops, 3, mean)
                    assert len(r) == 102 and r[1:] == [repr(float(v)) for v in feat[0]]
                    negative += sum(t.startswith("-") for t in r[1:])
        finally:
            m.close()
    assert negative > 0
    # the reference's own guard (assert numFeatures == featureBlob_size, calcSig_wOF.py:219-220): an uncaught AssertionError is exit
    # status 1 of the command; any way out must be non-zero, and nothing may have been written
    try:
        rc = run(tmp_path / "wrong", "--featureBlob_size", "1024")
    except AssertionError:
        rc = 1
    except SystemExit as e:
        rc = e.code
    assert rc not in (0, None)
    assert not [f for _, _, files in os.walk(str(tmp_path / "wrong")) for f in files if f.endswith(".csv")]


def test_caffenet_scores(tsn):
    """CaffeNet(scores=True): predict_* return the [10][101] float32 scores of the ten over-sampled crops -- what a ten-crop batched
    forward gives, bit for bit --, ``.data[0]`` is the default object's value, over_sample=False gives one row, an unknown score
    name raises; a default-built CaffeNet still returns None."""
    bi, net = tsn
    from video_query_algorithms_amd.tsn import caffe_net, frames
    rng = np.random.default_rng(41)
    for c, seed, mean in ((3, 2, net.RGB_MEAN), (10, 5, net.FLOW_MEAN)):
        g = bi.bn_inception(c)
        w = net.synthetic_weights(g, seed=seed)
        plain = caffe_net.CaffeNet(g, w, 0, max_crops=2)
        cn = caffe_net.CaffeNet(g, w, 0, max_crops=2, scores=True)                 # raised to the ten crops it needs
        direct = net.TsnNet(g, w, max_crops=10, feature_blob="fc-action")
        try:
            if c == 3:
                frame = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)]
                ten = frames.oversample(frame[0], (340, 256))
                call = lambda o, **kw: o.predict_single_frame(frame, "fc-action", frame_size=(340, 256), **kw)
            else:
                frame = [rng.integers(0, 256, (240, 320), dtype=np.uint8) for _ in range(10)]
                ten = frames.oversample_flow_stack(frame, (340, 256))
                call = lambda o, **kw: o.predict_single_flow_stack(frame, "fc-action", frame_size=(340, 256), **kw)
            assert call(plain) is None and set(plain._net.blobs) == {"global_pool"}
            ref0 = plain._net.blobs["global_pool"].data
            got = call(cn)
            assert got.shape == (10, 101) and got.dtype == np.float32
            _, want = direct.forward(ten, 1, mean)
            assert (_bits(got) == _bits(want)).all()
            assert cn._net.blobs["global_pool"].data.shape == (10, 1024, 1, 1) and cn._net.blobs["fc-action"].data.shape == (10, 101, 1, 1)
            assert cn._net.blobs["global_pool"].data[0].tobytes() == ref0[0].tobytes()
            assert (cn._net.blobs["fc-action"].data.reshape(10, 101) == got).all()
            one = call(cn, over_sample=False)
            assert one.shape == (1, 101) and (_bits(one[0]) == _bits(got[0])).all()
            assert cn._net.blobs["global_pool"].data.shape == (1, 1024, 1, 1) and cn._net.blobs["global_pool"].data[0].tobytes() == ref0[0].tobytes()
            with pytest.raises(KeyError):
                cn.predict_single_frame(frame, "no-such-blob") if c == 3 else cn.predict_single_flow_stack(frame, "no-such-blob")
        finally:
            plain.close()
            cn.close()
            direct.close()
