"""NumPy reference of nqk_topk_softmax / QModel.classify (shared by test_topk_host.py and
test_gpu_topk.py): stable argsort of the negated row, NumPy's own float32 Softmax gathered at
the selected columns, and the dequantize of oracle/nq_oracle.py restated."""
import numpy as np


def dequantize(q, scale, zp):
    """oracle/nq_oracle.py:dequantize: f32(f64(q - zp) * f64(scale)), zp a scalar or None"""
    q = np.asarray(q).astype(np.int64)
    if zp is not None:
        q = q - np.int64(zp)
    return (q.astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)


def topk_indices(y, k):
    y = np.asarray(y, dtype=np.float32)
    return np.argsort(-y, axis=-1, kind="stable")[..., :k].astype(np.int64)


def softmax(y):
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(all="ignore"):
        e = np.exp(y + (-y.max(-1, keepdims=True)))
        return e / e.sum(-1, keepdims=True)


def topk_softmax(y, k):
    """(idx, prob, value), each [..., k]"""
    y = np.asarray(y, dtype=np.float32)
    idx = topk_indices(y, k)
    return idx, np.take_along_axis(softmax(y), idx, -1), np.take_along_axis(y, idx, -1)


def brute_force_indices(row, k):
    """The definition, spelled out: not-NaN before NaN, larger value first with -0.0 == +0.0,
    equal values and NaNs by increasing column."""
    def key(c):
        v = float(row[c])
        if v != v:
            return (1, 0.0, c)
        return (0, -(v + 0.0) if v != 0.0 else 0.0, c)
    return np.array(sorted(range(len(row)), key=key)[:k], dtype=np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
