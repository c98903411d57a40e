"""Host only, no library: the registry of page-locked blocks (host_blocks.BlockRegistry) over a counting allocator -- what close()
must free, what a pool keeps, and that every allocation is freed exactly once."""
import ctypes
import gc

import numpy as np

from video_query_algorithms_amd.host_blocks import GRANULE, KINDS, BlockRegistry


class Heap:
    """A stand-in for vq_host_alloc / vq_host_free that counts, and refuses a second free of a block."""

    def __init__(self):
        self.live, self.allocated, self.freed = {}, [], []

    def alloc(self, nbytes):
        buf = (ctypes.c_ubyte * nbytes)()
        ptr = ctypes.addressof(buf)
        self.live[ptr] = buf
        self.allocated.append((ptr, nbytes))
        return ptr

    def free(self, ptr):
        del self.live[ptr]                                    # KeyError: freed twice, or never allocated
        self.freed.append(ptr)


def registry():
    heap = Heap()
    return heap, BlockRegistry(alloc=heap.alloc, free=heap.free)


def leave_idle(blocks, kind, sizes):
    """Take one block per entry of ``sizes`` at the same time, then release them all."""
    held = [blocks.take(kind, nbytes) for nbytes in sizes]
    del held


def test_a_block_returns_to_its_pool_when_its_last_view_dies():
    heap, blocks = registry()
    blk = blocks.take("fit", 1000)
    assert blk.nbytes == 1000 and heap.allocated == [(blk.ptr, GRANULE)]                       # sizes round up to 64 KiB
    raw = blk.bytes()
    assert raw.shape == (1000,) and raw.dtype == np.uint8 and raw.base is blk
    view = raw[64:128].view(np.float64)
    view[...] = 3.0
    ptr = blk.ptr
    del blk, raw
    gc.collect()
    assert blocks.idle("fit") == []                                                            # the view keeps the block out of the pool
    del view
    assert blocks.idle("fit") == [(ptr, GRANULE)] and not heap.freed
    again = blocks.take("fit", 70)                                                             # the same size class: the idle block, no allocation
    assert again.ptr == ptr and again.nbytes == 70 and len(heap.allocated) == 1 and blocks.idle("fit") == []
    other = blocks.take("grid", 70)                                                            # another kind has its own pools
    assert other.ptr != ptr and len(heap.allocated) == 2
    first, second = blocks.take("topk", 64), blocks.take("topk", 64)
    a, b = first.ptr, second.ptr
    del first
    del second
    assert blocks.take("topk", 64).ptr == b                                                    # last in, first out
    del again, other
    blocks.close()
    assert not heap.live and len(heap.freed) == len(heap.allocated) == 4 and a in heap.freed


def test_at_most_four_idle_blocks_per_kind_and_size():
    heap, blocks = registry()
    held = [blocks.take("update", GRANULE + 1) for _ in range(5)]
    assert [n for _p, n in heap.allocated] == [2 * GRANULE] * 5
    ptrs = [b.ptr for b in held]
    for _ in range(5):
        held.pop(0)
    assert [p for p, _n in blocks.idle("update")] == ptrs[:4] and heap.freed == [ptrs[4]]      # the fifth is freed
    leave_idle(blocks, "update", [5] * 5)                                                      # another size of the kind: four more
    assert len(blocks.idle("update")) == 8 and len(heap.freed) == 2
    blocks.close()
    assert not heap.live


def test_a_ninth_size_of_a_kind_drops_the_idle_blocks_of_the_old_sizes():
    heap, blocks = registry()
    for k in range(8):
        leave_idle(blocks, "view_round", [k * GRANULE + 1] * 2)
    assert len(blocks.idle("view_round")) == 16 and not heap.freed
    keep = blocks.take("fit", 1)
    del keep
    out = blocks.take("view_round", 3 * GRANULE + 1)                                           # a size it knows: nothing goes
    assert len(blocks.idle("view_round")) == 15 and not heap.freed
    ninth = blocks.take("view_round", 8 * GRANULE + 1)
    assert blocks.idle("view_round") == [] and len(heap.freed) == 15                           # the idle blocks of the eight old sizes
    assert len(blocks.idle("fit")) == 1                                                        # the other kinds keep theirs
    old = out.ptr
    del out                                                                                    # a block of a dropped size: freed, not pooled
    assert heap.freed[-1] == old and blocks.idle("view_round") == []
    p = ninth.ptr
    del ninth
    assert blocks.idle("view_round") == [(p, 9 * GRANULE)]
    blocks.close()
    assert not heap.live and sorted(heap.freed) == sorted(p for p, _n in heap.allocated)


def test_close_frees_every_idle_block_and_a_held_one_frees_itself():
    heap, blocks = registry()
    held = {}
    for i, kind in enumerate(KINDS):
        held[kind] = blocks.take(kind, 100 + i)
        leave_idle(blocks, kind, [7, GRANULE + 7, 7])                                          # idle blocks of two sizes of every kind
    assert all(len(blocks.idle(kind)) == 3 for kind in KINDS) and not heap.freed and not blocks.closed
    views = {kind: b.bytes()[:8] for kind, b in held.items()}
    ptrs = {kind: b.ptr for kind, b in held.items()}
    del held
    blocks.close()
    assert blocks.closed and all(blocks.idle(kind) == [] for kind in KINDS)
    assert len(heap.freed) == 3 * len(KINDS) and set(heap.live) == set(ptrs.values())          # the idle ones, and only they
    for kind in KINDS:
        views[kind][...] = 1                                                                   # still memory of ours
        del views[kind]
        assert ptrs[kind] in heap.freed and blocks.idle(kind) == []                            # freed when released, not pooled
    late = blocks.take("fit", 10)                                                              # a closed registry pools nothing any more
    del late
    assert not heap.live and blocks.idle("fit") == []
    assert sorted(heap.freed) == sorted(p for p, _n in heap.allocated)                         # every allocation freed exactly once


def test_an_unknown_kind_is_an_error():
    heap, blocks = registry()
    try:
        blocks.take("_fit_pools", 64)
    except KeyError:
        pass
    else:
        raise AssertionError("a kind the registry does not name must not make a pool")
    assert not heap.allocated


def test_a_constructor_that_fails_behind_the_create_call_still_destroys_the_handle(monkeypatch):
    """FeatureDB makes its registry before anything can fail, so close() -- from __del__ -- reaches vq_db_destroy for a handle whose
    constructor raised after vq_db_create (here: clip ids of the wrong shape).  The library is a stand-in."""
    from video_query_algorithms_amd import _lib, feature_db
    destroyed = []

    class Lib:
        def vq_db_destroy(self, handle):
            destroyed.append(handle.value)

    def create(name, *a):
        assert name == "vq_db_create", name
        a[-1]._obj.value = 77
    monkeypatch.setattr(feature_db, "call", create)
    monkeypatch.setattr(_lib, "load", lambda path=None: Lib())
    try:
        feature_db.FeatureDB(4, 2, 1, 256, clip_ids=[1, 2, 3])
    except ValueError:
        pass
    else:
        raise AssertionError("clip ids of the wrong shape must be refused")
    gc.collect()
    assert destroyed == [77]
