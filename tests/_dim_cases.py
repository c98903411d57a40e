"""The data of tests/test_dim_gpu.py and tests/_dim_child.py: rows drawn as in tests/test_sim_gpu.py (|N(0, 1)| in float32), stored in
the database's type (float16: rounded once -- the oracle is fed the rounded values), a presence mask that leaves every stream of
every clip at least one split, a search set of about two thirds of the rows, and a target that is a database row scaled by its
squared norm (target_clip.py:311-313), so similarities are O(1)."""
import numpy as np


def draw(rng, n, s, e, d, dtype):
    """-> x [n, s, e, d] in ``dtype``, present [n, s, e] uint8, rows (ascending, the search set), t [s, e, d] float64."""
    x = np.abs(rng.standard_normal((n, s, e, d))).astype(np.float32).astype(dtype)
    present = (rng.random((n, s, e)) > 0.2).astype(np.uint8)
    present[:, :, 0] = 1
    rows = np.flatnonzero(rng.random(n) < 0.67).astype(np.int64)
    if rows.size == 0:
        rows = np.array([n - 1], dtype=np.int64)
    return x, present, rows, target_of(x, int(rows[0]))


def target_of(x, row):
    r = x[row].astype(np.float64)
    return r / (r * r).sum(axis=-1, keepdims=True)


def padded(a, pitch):
    """[..., d] -> [..., pitch] of the same type, +0.0 in the pads."""
    out = np.zeros(a.shape[:-1] + (pitch,), dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def same(a, b):
    """Equal bit patterns up to the sign of zero and the payload of a NaN: ``==`` where both are numbers, NaN where either is."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
