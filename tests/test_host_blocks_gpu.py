"""GPU: every page-locked block a FeatureDB passes to the library comes from its registry (host_blocks.BlockRegistry) and goes with
the database -- each public call that takes a block runs once on a 200-row database (every partition in its one-workgroup form)
while the registry's allocator and free function and the library's own vq_host_alloc / vq_host_free are counted."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, S, E, D, G, T = 200, 2, 1, 256, 5, 4


def test_every_block_comes_from_the_registry_and_goes_with_the_database(gpu, monkeypatch):
    import video_query_algorithms_amd as vqa
    from video_query_algorithms_amd.host_blocks import KINDS
    lib = vqa.load_library()
    lib_allocs, lib_frees, reg_allocs, reg_frees, kinds = [], [], [], [], []
    real_alloc, real_free = lib.vq_host_alloc, lib.vq_host_free

    def lib_alloc(out, nbytes):                                                                # every page-locked allocation of the process
        rc = real_alloc(out, nbytes)
        lib_allocs.append(out._obj.value)
        return rc

    def lib_free(ptr):                                                                         # blocks of databases of earlier tests may go now too:
        if getattr(ptr, "value", ptr) in lib_allocs:                                           # only what was allocated in here counts
            lib_frees.append(getattr(ptr, "value", ptr))
        return real_free(ptr)
    gc.collect()
    monkeypatch.setattr(lib, "vq_host_alloc", lib_alloc)
    monkeypatch.setattr(lib, "vq_host_free", lib_free)

    rng = np.random.default_rng(3)
    x = np.abs(rng.standard_normal((N, S, E, D), dtype=np.float32))
    db = vqa.FeatureDB.from_arrays(x)
    db.define_search_rows("s", np.arange(3, N, 4, dtype=np.int64))                            # 50 rows
    blocks = db.blocks
    alloc, free, take = blocks._alloc, blocks._free, blocks.take
    blocks._alloc = lambda nbytes: (lambda ptr: (reg_allocs.append(ptr), ptr)[1])(alloc(nbytes))
    blocks._free = lambda ptr: (reg_frees.append(ptr), free(ptr))[1]
    blocks.take = lambda kind, nbytes: (kinds.append(kind), take(kind, nbytes))[1]

    t = np.stack([x[q].astype(np.float64) / np.sum(x[q].astype(np.float64) ** 2, axis=-1, keepdims=True) for q in range(3)])
    w = np.array([[1.0, 0.6], [1.0, 0.8], [1.0, 1.1]])
    bands = np.array([[0.8, 0.7]] * 3)
    cand, ths = np.stack([np.ones(G), np.linspace(0.5, 1.5, G)], axis=1), np.linspace(0.6, 0.9, T)
    rows, y = np.array([0, 7, 21, 40], dtype=np.int64), np.array([1.0, 0.0, 1.0, 0.0])
    results = [db.query_round(t[0], w[0], (0.8, 0.7))]
    results.append(db.query_round_batch(t, w, bands))
    results.append(db.query_round_batch_sets(t, w, ["s", None, "s"], bands))
    results.append(db.batch_round_fit([0, 2], [rows, rows[:2]], [y, y[:2]], [cand] * 2, [ths] * 2, [0.3] * 2))
    results.append(db.batch_round_grid([1], [rows], [cand]))
    avgs = db.batch_round_avg_rows([0, 1], [rows, rows])
    results.append(db.batch_round_rescore([1], w[1:2], bands[:1]))
    results.append(db.batch_round_update([0], [rows], [y], [cand], [ths], [0.3], [1], 1e-9, [0.35], [None], want_surface=True))
    results.append(db.batch_round_update_given([0, 1], [y, y], [np.array(a) for a in avgs], [cand] * 2, [ths] * 2, [0.3] * 2, [1, 1], 1e-9, [0.35, None],
                                               [None, np.array(avgs[1][:2])]))
    results.append(db.batch_round_topk(5))
    results.append(db.batch_targets([([3, 7, 11], [100, 101])], [[([0, 1, 2], [0, 1])]], [0.3]))
    results.append(avgs)
    assert set(kinds) == set(KINDS), set(KINDS) - set(kinds)                                   # every kind the registry names was used
    assert lib_allocs == reg_allocs and len(reg_allocs) > 0                                    # nothing outside the registry allocates
    assert lib_frees == reg_frees
    db.close()
    del results, avgs
    gc.collect()
    assert blocks.closed and all(blocks.idle(kind) == [] for kind in KINDS)
    assert lib_frees == reg_frees and sorted(reg_frees) == sorted(reg_allocs), (len(reg_allocs), len(reg_frees), len(lib_allocs), len(lib_frees))
