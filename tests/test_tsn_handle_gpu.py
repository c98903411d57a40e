"""What a TSN extractor handle owns on the device -- activation slots, weights and split-K scratch from the process-wide block pool, the
buffer host crops are staged in, the profiling ring, the sub-batch streams and their events -- through the ways it is made, grown,
replaced and released (csrc/vq_tsn.hip: struct vq_tsn, vq_tsn_create, vq_tsn_destroy, vq_tsn_forward, vq_tsn_set_profile).

The graph is the mini network of test_handles_are_thread_safe_and_do_not_leak (32 channels, 28 x 28, one 3x3 convolution to 64, max-pool
3/2, global pool; max_crops 6).  Every result is compared BIT FOR BIT with a fresh handle that did only that forward: whatever a handle
did before, whichever blocks it was given and however its forward is cut into sub-batches, the features are the same bits.  The
allocation-failure exits of vq_tsn_create are not walked here (no out-of-memory is provoked on a shared device)."""
import numpy as np
import pytest

import tsn_oracle as to

pytestmark = pytest.mark.gpu

MAX_CROPS = 6
SIZES = ((2, 2), (6, 3))                         # (crops, snippets per clip) of the forwards below


def _mini(bi):
    g = bi.Graph("mini", "data", (32, 28, 28))
    g.layers.append(bi.Layer("c", "Convolution", ["data"], ["c"], 64, 3, 1, 1))
    g.layers.append(bi.Layer("c_bn", "BN", ["c"], ["c_bn"]))
    g.layers.append(bi.Layer("c_relu", "ReLU", ["c_bn"], ["c_bn"]))
    g.layers.append(bi.Layer("p", "Pooling", ["c_bn"], ["p"], kernel=3, stride=2, pad=0, pool="MAX"))
    side = to.pool_out(28, 3, 2, 0)
    g.layers.append(bi.Layer("gp", "Pooling", ["p"], ["gp"], kernel=side, stride=1, pad=0, pool="AVE"))
    return g


class Case:
    pass


@pytest.fixture(scope="module")
def case(gpu):
    """The graph, its inputs and, per size, what a fresh handle that does only that forward returns (computed once, never written)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VQ_TUNE_CACHE", "0")              # every handle finds its tilings itself: the sweep's events are part of the handle
        for k in ("VQ_TSN_TILE", "VQ_TSN_SPLIT", "VQ_TSN_AUTOTUNE", "VQ_TSN_POISON", "VQ_TSN_GROUP", "VQ_TSN_GROUP_POOL", "VQ_TSN_SPLITK"):
            mp.delenv(k, raising=False)
        import video_query_algorithms_amd  # noqa: F401
        from video_query_algorithms_amd.tsn import bn_inception, net
        s = Case()
        s.net = net
        s.g = _mini(bn_inception)
        s.w = net.synthetic_weights(s.g, seed=4)
        s.crops = np.random.default_rng(2).integers(0, 256, (MAX_CROPS, 28, 28, 32), dtype=np.uint8)
        s.mean = np.full(32, 120.0, dtype=np.float32)
        s.want = {}
        for n, t in SIZES:
            m = s.open()
            s.want[n] = m.forward(s.crops[:n], t, s.mean)
            m.close()
            for a in s.want[n]:
                assert np.isfinite(a).all() and np.abs(a).max() > 0
                a.setflags(write=False)
        yield s


def _open(self, device=0):
    return self.net.TsnNet(self.g, self.w, max_crops=MAX_CROPS, device=device, feature_blob="gp")


def _same(self, got, n):
    feat, ps = got
    assert feat.tobytes() == self.want[n][0].tobytes(), "consensus features of %d crops differ from a fresh handle's" % n
    assert ps.tobytes() == self.want[n][1].tobytes(), "per-snippet features of %d crops differ from a fresh handle's" % n


Case.open = _open
Case.same = _same


def test_host_crops_of_growing_and_shrinking_batches(case):
    """Host crops of 2, then 6, then 2 snippets on one handle: the staging buffer is made for 2, replaced by a larger one for 6 and
    kept for the 2 that follow."""
    m = case.open()
    for n, t in ((2, 2), (6, 3), (2, 2)):
        case.same(m.forward(case.crops[:n], t, case.mean), n)
    m.close()


def test_profiling_ring_is_replaced_and_released_with_the_handle(case):
    """A ring of 2 event sets carries two forwards and yields the layer times; the ring is dropped (depth 0), made again with 3 sets,
    carries one forward, and the handle is closed with it alive."""
    m = case.open()
    m.set_profile(2)
    for _ in range(2):
        case.same(m.forward(case.crops, 3, case.mean), 6)
    names, kinds, ms, flops = m.layer_times()
    assert len(ms) == len(names) and np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0
    m.set_profile(0)
    case.same(m.forward(case.crops, 3, case.mean), 6)
    m.set_profile(3)
    case.same(m.forward(case.crops, 3, case.mean), 6)
    _, _, ms, _ = m.layer_times()
    assert np.isfinite(ms).all() and ms.sum() > 0
    m.close()


@pytest.mark.parametrize("split", ["1", "2", "2,1", "3"])
def test_sub_batch_streams_are_made_used_and_released(case, monkeypatch, split):
    """VQ_TSN_SPLIT = 1 (no extra stream), 2, 2,1 and 3: the handle makes its streams and join events, runs both sizes on them and
    is closed."""
    monkeypatch.setenv("VQ_TSN_SPLIT", split)
    m = case.open()
    for n, t in SIZES:
        case.same(m.forward(case.crops[:n], t, case.mean), n)
    m.close()


def test_a_handle_on_pooled_blocks_computes_the_same(case, monkeypatch):
    """A closed handle leaves its slots, weights and scratch in the block pool; the next handle of the same shape gets them as they
    are.  It is opened under VQ_TSN_POISON=1 (every slot NaN-filled before a forward): its features equal the first handle's."""
    m1 = case.open()
    first = m1.forward(case.crops, 3, case.mean)
    case.same(first, 6)
    m1.close()
    monkeypatch.setenv("VQ_TSN_POISON", "1")
    m2 = case.open()
    second = m2.forward(case.crops, 3, case.mean)
    assert second[0].tobytes() == first[0].tobytes() and second[1].tobytes() == first[1].tobytes()
    case.same(m2.forward(case.crops[:2], 2, case.mean), 2)
    m2.close()


def test_a_handle_of_a_second_device_is_destroyed_while_device_0_is_current(case):
    """The handle releases what it owns with ITS device current, whichever device the caller has selected."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    m = case.open(device=1)
    case.same(m.forward(case.crops, 3, case.mean), 6)
    torch.cuda.set_device(0)
    m.close()
    assert torch.cuda.current_device() == 0
    m0 = case.open()
    case.same(m0.forward(case.crops, 3, case.mean), 6)
    m0.close()
