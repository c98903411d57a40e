"""GPU: every op of both TSN networks in isolation at the product batch, every tiling on every real layer that can take it, and
every shipped tiling table at its own batch size.

The forward runs as the product runs it: the default handle (fused plan, Winograd, shipped tables, no tiling cache), 96 crops as
two sub-batches of 48 on two streams (the ``48p`` table).  Every op of ``m.plan.ops`` is then recomputed in fp64 from the device's
own input to that op (tests/_plan_walk.py: the graph's un-folded layers), on all 96 crops:

* convolutions (direct, Winograd, merged siblings, folded max pools, the commuted pool projections):
  |d| <= 2e-5 * max|y| over the op (the single-layer bound of tests/test_tsn_gpu.py) and, per output channel,
  |d| <= CHANNEL_REL * max(max|y_c|, 1e-2 * max|y|), never looser than the layer bound;
* max pools and the global average pool: bit-exact against ``pool_direct`` on the device's own fp32 input; consensus bit-exact.

Observed on an MI355X, all 96 crops, worst over the ops of a kind (max|d| / max|y| over the op; max over channels of
max|d_c| / max(max|y_c|, 1e-2 max|y|)), RGB | flow:
  stem (1)           6.2e-7 | 8.0e-7     channel 6.4e-7 | 1.4e-6
  pre_pool (4)       8.0e-7 | 6.4e-7     channel 5.1e-6 | 4.9e-6
  siblings (25)      1.6e-6 | 1.3e-6     channel 1.1e-5 | 1.3e-5
  direct (5)         1.3e-6 | 1.3e-6     channel 1.4e-5 | 1.3e-5     (the stride-2 3x3 layers and 5b/pool_proj)
  winograd (27)      7.0e-7 | 8.2e-7     channel 2.1e-5 | 1.3e-5
  linear (7)         1.5e-6 | 1.1e-6     channel 3.1e-6 | 3.6e-6     (the commuted projections before their pool)
  proj_pool (7)      6.2e-7 | 5.7e-7     channel 7.8e-6 | 4.2e-6
CHANNEL_REL = 8.5e-5 (tests/_plan_walk.py) is 4x the worst channel ratio; a change of 1e-4 of a channel's maximum fails it.
"""
import os

import numpy as np
import pytest

import _plan_walk as pw
import tsn_oracle as to

pytestmark = pytest.mark.gpu

N = 96                                          # the cfg-2 batch: 32 clips x 3 snippets
T = 3
PICK = list(range(N))                           # every crop: both sub-batches, their edges (47 | 48) and the ragged last M tiles
# every tiling of the direct kernel's table, in the external form [bm, bn, bk, pipe] (csrc/vq_tsn_conv.hip: kTiles)
DIRECT = [(bm, bn, bk, pipe) for pipe in (0, 1) for bm, bn in ((128, 128), (128, 96), (128, 64), (64, 128), (64, 64), (128, 32), (32, 128))
          for bk in (32, 16)] + [(64, 256, 16, 0), (64, 256, 8, 3), (64, 64, 8, 3), (128, 64, 8, 3)]
WINO = [(128, 32, 8, 2), (128, 64, 8, 2), (64, 32, 16, 2), (64, 64, 16, 2)]
PROBE = 2                                       # crops of the one-stream forwards that find which layers take a tiling


@pytest.fixture(scope="module")
def env(gpu):
    import torch
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VQ_TUNE_CACHE", "0")              # no tiling table of an earlier run: the shipped ones, or nothing
        for k in ("VQ_TSN_TILE", "VQ_TSN_SPLIT", "VQ_TSN_AUTOTUNE", "VQ_TSN_DEFAULT_TILES", "VQ_TSN_WINOGRAD", "VQ_TSN_WINO16",
                  "VQ_TSN_POISON", "VQ_TSN_GROUP", "VQ_TSN_SPLITK"):
            mp.delenv(k, raising=False)
        import video_query_algorithms_amd  # noqa: F401
        from video_query_algorithms_amd import _lib
        from video_query_algorithms_amd.tsn import bn_inception, net
        yield bn_inception, net, _lib
    torch.set_num_threads(threads)


class Case:
    pass


@pytest.fixture(scope="module", params=[3, 10], ids=["rgb", "flow"])
def case(env, request):
    """One network at the product batch, after the baseline forward: every slot of all 96 crops as the device left it."""
    bi, net, vlib = env
    s = Case()
    s.c = request.param
    s.g = bi.bn_inception(s.c)
    s.w = net.synthetic_weights(s.g, seed=2 if s.c == 3 else 5)
    s.mean = net.RGB_MEAN if s.c == 3 else net.FLOW_MEAN
    s.crops = np.random.default_rng(40 + s.c).integers(0, 256, (N, 224, 224, s.c), dtype=np.uint8)
    s.m = net.TsnNet(s.g, s.w, max_crops=N)
    assert s.m.default_tables == 4                              # 48, 24p, 96, 48p of the shipped tables
    s.base = s.m.layer_tiles(N // 2, paired=True)
    s.feat, s.ps = s.m.forward(s.crops, T, s.mean)
    assert (s.m.layer_tiles(N // 2, paired=True) == s.base).all()
    s.slots = {i: s.m.read_tensor(i, N) for i in range(1, len(s.m.plan.tensors))}
    s.data = s.m.read_blob("data", N)                           # the preprocessed input, space-to-depth packing undone
    s.vlib, s.net = vlib, net
    yield s
    s.m.close()


def _nchw(a, crops, coff, c, dtype=np.float64):
    return np.ascontiguousarray(a[crops][..., coff:coff + c].transpose(0, 3, 1, 2), dtype=dtype)


def test_every_op_against_fp64(case):
    s = case
    plan, m = s.m.plan, s.m
    wino = (s.vlib.VQ_OP_CONV_WINOGRAD, s.vlib.VQ_OP_CONV_WINOGRAD16)

    def read(slot, coff, c):
        return _nchw(s.data if slot == 0 else s.slots[slot], PICK, coff, c)

    stats = {}
    failures = []
    visited = outputs = 0
    for i, op in enumerate(plan.ops):
        if op.kind in ("maxpool", "gavgpool"):
            x = _nchw(s.slots[op.src], PICK, op.src_coff, op.cin, np.float32)
            want = to.pool_direct(x, op.k, op.stride, op.pad, "MAX" if op.kind == "maxpool" else "AVE")
            got = _nchw(s.slots[op.dst], PICK, op.dst_coff, op.cout, np.float32)
            ref = pw.op_reference(s.g, s.w, plan, op, read)[0].y
            if not ((got == want).all() and np.abs(got - ref).max() <= pw.LAYER_REL * np.abs(ref).max()):
                failures.append((op.name, "not bit-exact"))
            stats.setdefault(op.kind, [0, 0.0, 0.0])[0] += 1
            visited += 1
            outputs += 1
            continue
        for o in pw.op_reference(s.g, s.w, plan, op, read):
            got = read(o.slot, o.coff, o.c)
            ok, lr, cr = pw.check(got, o.y)
            if o.kind != "conv":
                kind = o.kind
            elif op.src == 0:
                kind = "stem"
            elif m.layer_op(i) in wino:
                kind = "winograd"
            elif op.pre_pool:
                kind = "pre_pool"
            else:
                kind = "siblings" if op.segments else "direct"
            st = stats.setdefault(kind, [0, 0.0, 0.0])
            st[0] += 1
            st[1], st[2] = max(st[1], lr), max(st[2], cr)
            if not ok:
                failures.append((o.name, lr, cr))
            outputs += 1
        visited += 1
    print("\n%s: %d ops, %d outputs checked on %d crops" % ("rgb" if s.c == 3 else "flow", visited, outputs, len(PICK)))
    for kind, (n, lr, cr) in sorted(stats.items()):
        print("  %-9s %3d  layer %.2e  channel %.2e" % (kind, n, lr, cr))
    assert visited == len(plan.ops) == 55
    assert outputs == 69 + 7 + 3 + 1                            # every convolution of the graph, the 7 commuted pools, 3 max pools, the global pool
    assert not failures, failures
    # the per-snippet features are the feature slot; the consensus is the fp64 mean of them
    assert (s.ps == s.slots[plan.feature_slot].reshape(N, -1)).all()
    assert (s.feat == to.consensus(s.ps, T)).all()
    # negative control: the reference of a real layer from its input with two crops swapped must fail the check
    op = next(o for o in plan.ops if o.segments)

    def swapped(slot, coff, c):
        x = read(slot, coff, c)
        x[[0, 1]] = x[[1, 0]]
        return x
    for o in pw.op_reference(s.g, s.w, plan, op, swapped):
        assert not pw.check(read(o.slot, o.coff, o.c), o.y)[0], o.name


def _legal(s):
    """{tiling: [layers that take it]}: the library decides -- one layer changed at a time, in one-stream forwards of PROBE crops (a
    direct tiling without a kernel for the layer fails the launch; a Winograd form the layer lacks is refused when installed)."""
    m, vlib = s.m, s.vlib
    n_ops = len(m.plan.ops)
    direct = [i for i in range(n_ops) if m.layer_op(i) == vlib.VQ_OP_CONV]
    wino = [i for i in range(n_ops) if m.layer_op(i) in (vlib.VQ_OP_CONV_WINOGRAD, vlib.VQ_OP_CONV_WINOGRAD16)]
    assert len(direct) == 17 and len(wino) == 27
    m.set_split(PROBE, False)
    legal = {}
    for t in DIRECT + WINO:
        legal[t] = []
        for i in (wino if t in WINO else direct):
            tab = s.base.copy()
            tab[i] = t
            try:
                m.set_layer_tiles(PROBE, tab, paired=False)
                m.forward(s.crops[:PROBE], 1, s.mean)
            except vlib.VqError:
                continue
            legal[t].append(i)
    m.set_split(PROBE, None)
    return legal


def _bits(a):
    return a.view(np.uint32)


def test_every_tiling_on_every_real_layer_gives_the_same_bits(case):
    """Baseline: the shipped 48p table.  For each tiling, every layer that takes it gets it (the others keep their baseline tile);
    the table must read back as installed, and every output bit of the changed layers and every per-snippet feature must equal
    the baseline.  On the pooled-input layers conv_launch runs a tiling without a pooled kernel as the pooled BK = 16 tiling of its
    shape (same bits), and the RGB stem runs its BK = 16 sibling: such layers count as taking the tiling."""
    s = case
    m = s.m
    legal = _legal(s)
    counts = {}
    try:
        for t in DIRECT + WINO:
            layers = legal[t]
            counts[t] = len(layers)
            if not layers:
                continue
            tab = s.base.copy()
            tab[layers] = t
            m.set_layer_tiles(N // 2, tab, paired=True)
            feat, ps = m.forward(s.crops, T, s.mean)
            assert (m.layer_tiles(N // 2, paired=True) == tab).all(), t
            assert (_bits(ps) == _bits(s.ps)).all() and (feat == s.feat).all(), t
            dsts = sorted({sg.dst for i in layers for sg in (m.plan.ops[i].segments or [m.plan.ops[i]])})
            for d in dsts:
                assert (_bits(m.read_tensor(d, N)) == _bits(s.slots[d])).all(), (t, d)
    finally:
        m.set_layer_tiles(N // 2, s.base, paired=True)
    print("\n%s: layers per tiling %s" % ("rgb" if s.c == 3 else "flow", {"x".join(map(str, t)): n for t, n in counts.items()}))
    assert all(counts[t] >= 1 for t in DIRECT + WINO), counts
    assert all(counts[t] == 27 for t in WINO[:2])                   # the 32-tile forms run on every Winograd layer


def test_every_shipped_table_at_its_own_batch(case):
    """Each of the 12 shipped tables of the network in the forward that uses it -- a plain table N: N crops on one stream; Np: 2N
    crops as two sub-batches -- gives the per-snippet features of the same crops run through 48-crop forwards, bit for bit."""
    s = case
    net = s.net
    tables = net._default_tiles()[s.m.graph_key]
    sizes = sorted({int(k.rstrip("p")) * (2 if k.endswith("p") else 1) for k in tables})
    assert len(tables) == 12 and sizes == [48, 96, 224, 400, 448, 800]
    top = 17 * 48                                                   # 816 crops: whole 48-crop forwards cover the largest size
    crops = np.random.default_rng(7 + s.c).integers(0, 256, (top, 224, 224, s.c), dtype=np.uint8)
    m = net.TsnNet(s.g, s.w, max_crops=top)
    ran = []
    try:
        assert m.default_tables == 12
        ref = np.concatenate([m.forward(crops[i:i + 48], 8, s.mean)[1] for i in range(0, top, 48)])
        for name in sorted(tables, key=lambda k: (int(k.rstrip("p")), k)):
            paired = name.endswith("p")
            sub = int(name.rstrip("p"))
            n = 2 * sub if paired else sub
            assert (m.layer_tiles(sub, paired=paired) == np.array(tables[name])).all(), name
            m.set_split(n, paired)
            feat, ps = m.forward(crops[:n], 8, s.mean)
            m.set_split(n, None)
            assert (sub, paired, False) in m.tile_tables(), name        # the shipped table, not a borrowed or a tuned one
            assert (_bits(ps) == _bits(ref[:n])).all(), name
            assert (feat == to.consensus(ps, 8)).all(), name
            ran.append("%s@%d" % (name, n))
    finally:
        m.close()
    print("\n%s: shipped tables run at their own batch: %s" % ("rgb" if s.c == 3 else "flow", ", ".join(ran)))
    assert len(ran) == 12
