"""The page-locked host blocks a database handle passes to the library, pooled: one registry per handle, every kind of block in it."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib

KINDS = ("round", "batch_round", "view_round", "fit", "grid", "update", "topk", "targets")
IDLE_PER_SIZE, SIZES_PER_KIND, GRANULE = 4, 8, 65536


def _host_alloc(nbytes: int) -> int:
    p = C.c_void_p()
    _lib.call("vq_host_alloc", C.byref(p), nbytes)
    return p.value


def _host_free(ptr: int):
    _lib.load().vq_host_free(C.c_void_p(ptr))


class _RoundBlock:
    """One page-locked host block of vq_db_query_round (include/vq_amd.h) or of a batched call, exposed to numpy: ``nbytes`` as asked
    for, at ``ptr``.  The arrays a call hands out are views of it; when the last of them is gone the block goes back to its
    registry (or is freed if that is closed)."""

    def __init__(self, ptr: int, nbytes: int, registry: "BlockRegistry", kind: str, size: int):
        self.ptr, self.nbytes, self._home = ptr, nbytes, (registry, kind, size)
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}

    def bytes(self) -> np.ndarray:
        return np.asarray(self)                               # its .base is self: views of it keep the block out of the pool

    def __del__(self):
        try:
            registry, kind, size = self._home
            registry._give_back(kind, size, self.ptr)         # reborn as a fresh _RoundBlock by the next take
        except Exception:
            pass


class BlockRegistry:
    """Every pool of page-locked blocks of one handle: per kind (``KINDS``) and size -- rounded up to 64 KiB -- at most 4 idle blocks;
    a kind that meets a ninth size drops the idle blocks of its old sizes.  One rule for every kind: the blocks of one-query and
    whole-database rounds, once allocated exact and pooled per number of queries without a limit, round up and fall under the
    nine-sizes rule like the rest (16 numbers of queries can make more than 8 sizes).  Made with the handle, so the first calls of
    two threads share it.  ``take`` needs no lock of the caller's: the registry has its own (re-entrant, because a block may be collected --
    and come back -- while this thread is inside ``take``); the allocator and the free function run outside it."""

    def __init__(self, alloc=None, free=None):
        self._alloc, self._free = alloc or _host_alloc, free or _host_free
        self._idle = {kind: {} for kind in KINDS}             # kind -> {size: [ptr, ...]}, last in, first out
        self._lock = threading.RLock()
        self.closed = False

    def take(self, kind: str, nbytes: int) -> _RoundBlock:
        """A block of ``nbytes`` bytes of ``kind``: the idle one returned last, or a new one."""
        size = (nbytes + GRANULE - 1) // GRANULE * GRANULE or GRANULE
        dropped = ()
        with self._lock:
            sizes = self._idle[kind]
            stack = sizes.get(size)
            if stack is None:
                if len(sizes) >= SIZES_PER_KIND:              # many sizes: the idle blocks of the old ones go
                    dropped = [p for old in sizes.values() for p in old]
                    sizes.clear()
                stack = sizes[size] = []
            ptr = stack.pop() if stack else None
        for p in dropped:
            self._free(p)
        return _RoundBlock(self._alloc(size) if ptr is None else ptr, nbytes, self, kind, size)

    def idle(self, kind: str) -> list:
        """The idle blocks of ``kind`` as (ptr, size)."""
        with self._lock:
            return [(p, size) for size, stack in self._idle[kind].items() for p in stack]

    def _give_back(self, kind: str, size: int, ptr: int):
        with self._lock:
            stack = None if self.closed else self._idle[kind].get(size)         # a size the kind dropped since: not pooled again
            keep = stack is not None and len(stack) < IDLE_PER_SIZE
            if keep:
                stack.append(ptr)
        if not keep:
            self._free(ptr)

    def close(self):
        """Free every idle block of every kind; a block still referenced by result arrays frees itself when they go."""
        with self._lock:
            self.closed = True
            idle = [p for sizes in self._idle.values() for stack in sizes.values() for p in stack]
            for sizes in self._idle.values():
                sizes.clear()
        for p in idle:
            self._free(p)
