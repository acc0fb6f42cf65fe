"""NumPy restatement of the weight clipping search (Model.quantize(weight_clip="mse")): the specification.
Nothing here imports numpy_quant.  The eligible weights are tests/_perchannel_ref.py's, at the width of
tests/_mixed_ref.py; every formula is the reference's quantize / dequantize without a zero point.

Ratios     ratio[g] = f32(1 - 0.5 g / steps), g < steps <= 64, the factor in float64
Candidate  s = f32(s0[n] * ratio[g]); s0 the column's scale (column_scales) or the tensor's, broadcast
Element    q = rint(clip(f32(w / s), f32(lo), f32(hi))), dq = f32(f64(q) f64(s)), d = f64(w) - f64(dq)
Error      err[g][n] = the float64 sum of d d over the column: partial j (j < 64) adds rows j, j + 64, ..
           in increasing order to +0.0; then p[j] = p[j] + p[j ^ m] for all j at once, m = 32, .., 1
Choice     the first g with the smallest err[g][n] (a later g wins only by err < best); per tensor the
           same rule on err.sum(axis=1), and the scale f32(s0 ratio[g])
Kept       a column whose s0 is 0 or not finite: scale = s0, index 0, err +0.0
"""
import numpy as np

import _mixed_ref as M
import _perchannel_ref as P
from oracle import nq_oracle as O


def ratios(steps):
    return (1.0 - 0.5 * np.arange(steps, dtype=np.float64) / float(steps)).astype(np.float32)


def ordered_sum(sq):
    rows, n = sq.shape
    rounds = -(-rows // 64)
    padded = np.zeros((rounds * 64, n), np.float64)
    padded[:rows] = sq
    p = np.zeros((64, n), np.float64)
    for r in range(rounds):
        p = p + padded[r * 64:(r + 1) * 64]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ m]
    return p[0]


def first_minimum(err):
    best = err[0].copy()
    index = np.zeros(err.shape[1:], np.int32)
    for g in range(1, err.shape[0]):
        better = err[g] < best
        best = np.where(better, err[g], best)
        index = np.where(better, np.int32(g), index)
    return index


def search_cols(w, s0, ratio, bit_width):
    """(scale float32 [N], index int32 [N], err float64 [G, N]) of float32 w [rows, N]."""
    w, s0, ratio = np.asarray(w), np.asarray(s0), np.asarray(ratio)
    assert w.dtype == s0.dtype == ratio.dtype == np.float32 and w.ndim == 2 and s0.shape == (w.shape[1],)
    lo, hi = O.qrange(bit_width)
    err = np.zeros((ratio.shape[0], w.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        cand = s0[None, :] * ratio[:, None]
        assert cand.dtype == np.float32
        for g in range(ratio.shape[0]):
            s = cand[g]
            q = np.rint(np.minimum(np.maximum(np.true_divide(w, s[None, :]), np.float32(lo)), np.float32(hi)))
            dq = (q.astype(np.float64) * s.astype(np.float64)[None, :]).astype(np.float32)
            d = w.astype(np.float64) - dq.astype(np.float64)
            err[g] = ordered_sum(d * d)
    kept = (s0 == 0) | ~np.isfinite(s0)
    err[:, kept] = 0.0
    index = first_minimum(err)
    scale = np.where(kept, s0, cand[index, np.arange(w.shape[1])])
    return scale.astype(np.float32), index, err


def search_tensor(w, s0, ratio, bit_width):
    """(scale float32 scalar, g) of float32 w [rows, N] with the tensor's scale s0."""
    s0 = np.float32(s0)
    _, _, err = search_cols(w, np.full(w.shape[1], s0, np.float32), ratio, bit_width)
    g = int(first_minimum(err.sum(axis=1)[:, None])[0])
    return s0 * np.asarray(ratio, np.float32)[g], g


def calibrate(graph, calibration_inputs, bit_width=8, weight_bit_width=None, per_channel=False, steps=64):
    """Model.quantize(..., weight_clip="mse", clip_steps=steps): tests/_mixed_ref.py's calibration, then
    every eligible weight again with its searched scale and the biases of their Gemms with s_x s_w."""
    w = M.weight_width(bit_width, weight_bit_width)
    qp, qconst, axes = M.calibrate(graph, calibration_inputs, bit_width, weight_bit_width, per_channel)
    r = ratios(steps)
    for name, axis in axes.items():
        arr = graph.constants[name]
        cols = arr if axis == 1 else np.ascontiguousarray(arr.T)
        if per_channel:
            s = search_cols(cols, qp[name].scale, r, w)[0]
            q = P.quantize_cols(arr, s, w, axis)
        else:
            s = search_tensor(cols, qp[name].scale, r, w)[0]
            q = O.quantize(arr, w, s, None)
        qp[name] = O.QParams(s, None)
        qconst[name] = O.Q(q, w, s, None)
    for _, op, _, ins, _ in graph.nodes:
        if op == "Gemm" and ins[1] in axes:
            s_x, s_w = qp[ins[0]].scale, qp[ins[1]].scale
            if per_channel:
                bscale = (np.float32(s_x) * s_w).astype(np.float32)
                qb = P.quantize_cols(graph.constants[ins[2]], bscale, 4 * bit_width)
            else:
                bscale = s_x * s_w
                qb = O.quantize(graph.constants[ins[2]], 4 * bit_width, bscale, None)
            qp[ins[2]] = O.QParams(bscale, None)
            qconst[ins[2]] = O.Q(qb, 4 * bit_width, bscale, None)
    return qp, qconst, axes
