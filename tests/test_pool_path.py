"""The pooling path of the inception modules (csrc/vq_tsn_kernels.h: pool_unit for the windows (3, 1, 1) and (3, 2, 0), pool_one for every
other window): bit-exact against ``tsn_oracle.pool_direct`` on the device's own input blob, riding in a Winograd launch and as a launch
of its own (VQ_TSN_GROUP_POOL=0), plus the host-only proof that the reciprocal form of ``a / 9.0f`` returns the division's bits.

The graph of a case is a cut-down inception module on a 32-channel input of h x w pixels, 3 crops:

    a    3x3/1/1 conv, 32 channels                                   x0 = Concat[a, c]: the pooled blob c sits at channel offset 32 of a
    c    1x1 conv, C channels (+ ReLU, or none: the negative case)    slot of 32 + C channels
    w3   3x3/1/1 conv on a;  w4  3x3/1/1 conv on w3                  the Winograd launches the pooling layers ride in
    p    the pooling layer under test, on c                          (AVE (3, 1, 1) "proj" cases: followed by a 1x1 projection + BN + ReLU,
    q    the same pooling on w3                                       which the plan commutes: the pool runs on the projected channels and
    out  Concat[q, p]                                                 adds the folded bias and the ReLU)
    gp   MAX pool over the whole of `out` (the 1x1 feature blob)     p writes at channel offset 32 of a slot of 32 + C (or 32 + 32) channels

Every pooling op of the plan (p, q and gp -- gp and the (2, 2, 0) / (3, 1, 0) windows take the generic path) is recomputed from the
slot the device read.  ``==`` on fp32 values: equal bits, +0 and -0 aside (what tests/test_tsn_gpu.py::test_pooling_is_bit_exact asks);
VQ_TSN_POISON fills every slot with NaN patterns first, so an element a kernel fails to write cannot pass.
Sizes: 1, 2 and 3 clip the window on both sides; 9 with stride 2 clips the last ceil-mode window; 7 x 9 and 14 x 3 are not square;
C = 4, 32, 320 puts 1, 8, 80 channel quads in a pixel (a 1 024-output workgroup then straddles pixels, rows and the 3 crops).
A (3, 2, 0) window has no output on a 1-pixel map (Caffe's size rule gives 0), so that window starts at size 2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import tsn_oracle as to

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "video-query-algorithms_amd", "csrc")
N = 3


# ------------------------------------------------------------------------------------------------------------------------------
# host only: div9(a) == a / 9.0f for all 2^32 floats
# ------------------------------------------------------------------------------------------------------------------------------
DIV9_MAIN = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include <atomic>
#include "vq_div9.h"
int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 8;
    std::atomic<uint64_t> bad{0}, seen{0};
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            uint64_t b = 0, n = 0;
            const uint64_t lo = (1ull << 32) * t / T, hi = (1ull << 32) * (t + 1) / T;
            for (uint64_t x = lo; x < hi; ++x) {
                const uint32_t u = (uint32_t)x;
                uint32_t w, g;
                float a;
                memcpy(&a, &u, 4);
                const float want = a / 9.0f, got = vq::div9(a);
                memcpy(&w, &want, 4);
                memcpy(&g, &got, 4);
                b += (w != g) & !((want != want) & (got != got));      // NaN for NaN: any payload
                ++n;
            }
            bad += b;
            seen += n;
        });
    for (auto& x : th) x.join();
    printf("%llu %llu\n", (unsigned long long)seen.load(), (unsigned long long)bad.load());
    return 0;
}
"""


def test_div9_returns_the_bits_of_the_division_for_every_float(tmp_path):
    """All 2^32 inputs (zeros, subnormals, infinities, NaNs included) through csrc/vq_div9.h, the header the kernel compiles, against
    ``a / 9.0f``: zero mismatches.  The program is built with the host compiler's FMA instructions and no contraction of its own."""
    src = tmp_path / "div9_all.cc"
    src.write_text(DIV9_MAIN)
    exe = tmp_path / "div9_all"
    subprocess.run([os.environ.get("CXX", "g++"), "-O3", "-std=c++17", "-march=native", "-ffp-contract=off", "-pthread", "-I" + CSRC,
                    str(src), "-o", str(exe)], check=True)
    threads = max(1, min(16, os.cpu_count() or 1))
    out = subprocess.run([str(exe), str(threads)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == 1 << 32
    assert int(out[1]) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tsn(gpu):
    import video_query_algorithms_amd  # noqa: F401
    from video_query_algorithms_amd.tsn import bn_inception, net
    return bn_inception, net


def _module(bi, h, w, c, kind, k, s, p, relu, proj):
    g = bi.Graph("pool_module", "data", (32, h, w))

    def conv(name, bottom, n, kk, pad, act=True):
        g.layers.append(bi.Layer(name, "Convolution", [bottom], [name], n, kk, 1, pad))
        g.layers.append(bi.Layer(name + "_bn", "BN", [name], [name + "_bn"]))
        if act:
            g.layers.append(bi.Layer(name + "_relu", "ReLU", [name + "_bn"], [name + "_bn"]))
        return name + "_bn"

    a = conv("a", "data", 32, 3, 1)
    c_bn = conv("c", "data", c, 1, 0, act=relu)
    g.layers.append(bi.Layer("x0", "Concat", [a, c_bn], ["x0"]))
    w3 = conv("w3", a, 32, 3, 1)
    conv("w4", w3, 32, 3, 1)
    g.layers.append(bi.Layer("p", "Pooling", [c_bn], ["p"], kernel=k, stride=s, pad=p, pool=kind))
    top = conv("proj", "p", 32, 1, 0) if proj else "p"
    g.layers.append(bi.Layer("q", "Pooling", [w3], ["q"], kernel=k, stride=s, pad=p, pool=kind))
    g.layers.append(bi.Layer("out", "Concat", ["q", top], ["out"]))
    ho, wo = to.pool_out(h, k, s, p), to.pool_out(w, k, s, p)
    kk = max(ho, wo)
    g.layers.append(bi.Layer("gp", "Pooling", ["out"], ["gp"], kernel=kk, stride=kk, pad=0, pool="MAX"))
    return g


def _nchw(a, coff, c):
    return np.ascontiguousarray(a[..., coff:coff + c].transpose(0, 3, 1, 2))


SIZES = [(1, 1), (2, 2), (3, 3), (7, 7), (9, 9), (14, 14), (7, 9), (14, 3)]
CHANNELS = [4, 32, 320]


def _cases():
    """(kind, k, s, p, h, w, C, variant).  Every (kind, window) meets every size, and C cycles so that each meets 4, 32 and 320 on clipped
    and on unclipped maps.  Variants: "relu" (post-ReLU input), "neg" (MAX on a blob that is negative everywhere), "proj" (AVE with the
    commuted-projection bias and ReLU; the projection reads its source at a channel offset, which the direct kernel takes from 32 channels up)."""
    out = []
    n = 0
    for kind in ("MAX", "AVE"):
        for k, s, p in ((3, 1, 1), (3, 2, 0), (2, 2, 0), (3, 1, 0)):
            for h, w in SIZES:
                if min(to.pool_out(h, k, s, p), to.pool_out(w, k, s, p)) < 1:
                    continue                                    # no output at all: not a layer
                if kind == "AVE" and p == 0 and h == k and w == k:
                    continue                                    # the window is the map: the plan makes it a global average pool (another kernel)
                if (k, s, p) in ((2, 2, 0), (3, 1, 0)) and (h, w) not in ((3, 3), (9, 9), (7, 9)):
                    continue                                    # the generic path: unchanged code, three sizes
                c = CHANNELS[n % 3]
                n += 1
                out.append((kind, k, s, p, h, w, c, "relu"))
                if kind == "MAX" and (k, s, p) in ((3, 1, 1), (3, 2, 0)) and (h, w) in ((2, 2), (9, 9), (7, 9)):
                    out.append((kind, k, s, p, h, w, c, "neg"))
                if kind == "AVE" and (k, s, p) == (3, 1, 1) and (h, w) in ((1, 1), (3, 3), (14, 14), (7, 9)):
                    out.append((kind, k, s, p, h, w, 32 if c == 4 else c, "proj"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k,s,p,h,w,c,variant", _cases())
def test_pooling_bits_on_both_routes(tsn, monkeypatch, kind, k, s, p, h, w, c, variant):
    bi, net = tsn
    g = _module(bi, h, w, c, kind, k, s, p, relu=variant != "neg", proj=variant == "proj")
    wts = net.synthetic_weights(g, seed=11)
    if variant == "neg":                                        # a pre-ReLU blob that is negative everywhere: about -1 +- 0.3
        wts["c_bn"]["scale"] = (wts["c_bn"]["scale"] * 1e-3).astype(np.float32)
        wts["c_bn"]["shift"] = np.full(c, -1.0, dtype=np.float32)
    crops = np.random.default_rng(100 * h + w).integers(0, 256, (N, h, w, 32), dtype=np.uint8)
    mean = np.full(32, 120.0, dtype=np.float32)
    monkeypatch.setenv("VQ_TSN_POISON", "1")
    monkeypatch.setenv("VQ_TUNE_CACHE", "0")
    got = {}
    for route in ("1", "0"):
        monkeypatch.setenv("VQ_TSN_GROUP_POOL", route)
        m = net.TsnNet(g, wts, max_crops=N, feature_blob="gp", keep=("w4_bn",))
        try:
            ops = m.plan.ops
            names = [o.name for o in ops]
            items, _ = m.launch_items()
            wino = {items[names.index(x)] for x in ("a", "w3", "w4")}
            for name in ("p", "q"):                             # riding in a Winograd launch, or in a launch of its own
                assert (items[names.index(name)] in wino) == (route == "1"), (name, route)
            m.forward(crops, 1, mean)
            slots = {}
            pools = [o for o in ops if o.kind in ("maxpool", "avgpool")]
            assert [o.name for o in pools] == ["p", "q", "gp"] or [o.name for o in pools] == ["q", "p", "gp"]
            for op in pools:
                for sl in (op.src, op.dst):
                    if sl not in slots:
                        slots[sl] = m.read_tensor(sl, N)
                x = _nchw(slots[op.src], op.src_coff, op.cin)
                assert np.isfinite(x).all()
                if op.name == "p":
                    t_in, t_out = m.plan.tensors[op.src], m.plan.tensors[op.dst]
                    assert (op.dst_coff, t_out.c) == (32, 32 + op.cout)             # inside a wider concat slot
                    if variant == "proj":
                        assert op.bias_from == ("proj", "proj_bn") and op.relu and op.cin == 32
                    else:
                        assert (op.src_coff, t_in.c, op.cin) == (32, 32 + c, c)     # a source at a channel offset
                    if variant == "neg":
                        assert x.max() < 0
                want = to.pool_direct(x, op.k, op.stride, op.pad, "MAX" if op.kind == "maxpool" else "AVE")
                if op.bias_from is not None:
                    _, b = net.fold_bn(wts[op.bias_from[0]], wts[op.bias_from[1]])
                    want = want + b[None, :, None, None]
                    if op.relu:
                        want = np.maximum(want, np.float32(0))
                y = _nchw(slots[op.dst], op.dst_coff, op.cout)
                assert want.dtype == np.float32 and y.shape == want.shape
                assert (y == want).all(), (op.name, route, int((y != want).sum()))
                got[(route, op.name)] = y
        finally:
            m.close()
    for name in ("p", "q", "gp"):
        assert (got[("1", name)].view(np.uint32) == got[("0", name)].view(np.uint32)).all(), name
