"""NumPy restatement of per-column weight scales (QModel.per_channel): the specification.

The reference quantizes every constant with one scale (numpy_quant/model.py:357-365).  Here an
eligible weight gets one scale per output column; every formula is the reference's
(numpy_quantization.py:7-72, restated in oracle/nq_oracle.py) with a scale vector s[n] over the
output columns in the scalar's place.  Nothing here imports numpy_quant.

Eligible   a 2-D constant each consumer of which is a MatMul taking it as input 1 (columns on
           the last axis) or a Gemm taking it as its weight, input 1 (the last axis; axis 0 with
           transB), all naming the same axis.  Everything else keeps its one scale.
Scale      s_w[n], _ = quant_parameters(min(0, min_k W[k, n]), max(0, max_k W[k, n]), bw, False)
Weight     q[k, n] = quantize(W[k, n], s_w[n], None, bw), element by element
q_matmul   unchanged; its output carries s[n] = f32(s_a) * f32(s_w[n])
Dequantize f32(f64(acc - zpt) * f64(s[n])); requantize goes on from there as before
Gemm bias  quantized at 4 * bw with bscale[n] = s_x * s_w[n], element by element
"""
import numpy as np

from oracle import nq_oracle as O


# ----------------------------------------------------------------------------- definition
def consumers(graph):
    """{value name: [(op, attrs, input index)]} over the graph's nodes."""
    out = {}
    for _, op, attrs, ins, _ in graph.nodes:
        for k, name in enumerate(ins):
            out.setdefault(name, []).append((op, attrs, k))
    return out


def eligible_axis(graph, name, cons=None):
    """The output-column axis (0 or 1) of constant `name`, or None when it keeps one scale."""
    arr = graph.constants.get(name)
    if arr is None or arr.ndim != 2 or arr.size == 0:
        return None
    cons = consumers(graph) if cons is None else cons
    axes = set()
    uses = cons.get(name, [])
    if not uses:
        return None
    for op, attrs, k in uses:
        if op not in ("MatMul", "Gemm") or k != 1:
            return None
        axes.add(0 if op == "Gemm" and attrs.get("transB") else 1)
    return axes.pop() if len(axes) == 1 else None


def column_scales(w, axis, bit_width):
    """float32 [N] of a 2-D float32 weight whose output columns lie on `axis`."""
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.ndim == 2
    red = 1 - axis
    zero = np.float32(0)
    mn = np.minimum(w.min(axis=red), zero)
    mx = np.maximum(w.max(axis=red), zero)
    return np.array([O.quant_parameters(mn[n], mx[n], bit_width, False)[0] for n in range(mn.shape[0])],
                    dtype=np.float32)


def _along(s, axis, ndim=2):
    """The vector shaped to broadcast along `axis`."""
    shape = [1] * ndim
    shape[axis] = -1
    return np.asarray(s, np.float32).reshape(shape)


def quantize_cols(x, s, bit_width, axis=-1):
    """quantize (numpy_quantization.py:24-34, no zero point) with the scale of each element's
    index on `axis`: clip(f32(x / s[n]), f32(lo), f32(hi)), rint, int64."""
    lo, hi = O.qrange(bit_width)
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        t = np.true_divide(x, _along(s, axis % x.ndim, x.ndim))
        assert t.dtype == np.float32
        u = np.minimum(np.maximum(t, np.float32(lo)), np.float32(hi))
        return np.rint(u).astype(np.int64)


def dequantize_cols(q, s, zpt):
    """f32(f64(q - zpt) * f64(s[n])), n the index on the last axis."""
    centred = q if zpt is None else (q - zpt)
    prod = np.asarray(centred, np.int64).astype(np.float64) * np.asarray(s, np.float32).astype(np.float64)
    return prod.astype(np.float32)


def requantize_cols(acc, s, zpt, res_scale, res_zp, bit_width):
    """requantize (numpy_quantization.py:64-72) from dequantize_cols on."""
    lo, hi = O.qrange(bit_width)
    d = dequantize_cols(acc, s, zpt)
    with np.errstate(all="ignore"):
        r = np.float32(1) / np.float32(res_scale)
        v = (r * d).astype(np.float32)
        if res_zp is None:
            u = np.rint(v)
            return np.minimum(np.maximum(u, np.float32(lo)), np.float32(hi)).astype(np.int64)
        u = np.rint(np.asarray(res_zp).astype(np.float64) + v.astype(np.float64))
        return np.minimum(np.maximum(u, np.float64(lo)), np.float64(hi)).astype(np.int64)


def int_matmul(a, b):
    """The exact integer product through float64 BLAS (|acc| < 2^53 for every bit width <= 16
    and K < 2^21), checked on a slice against NumPy's int64 matmul."""
    acc = np.matmul(a.astype(np.float64), b.astype(np.float64)).astype(np.int64)
    sa, sb = a[..., :3, :], b[..., :, :5]
    assert np.array_equal(acc[..., :3, :5], np.matmul(sa.astype(np.int64), sb.astype(np.int64)))
    return acc


def q_matmul(a, s_a, zp_a, b, s_b, zp_b):
    """numpy_quantization.py:44-61, unchanged: s_b may be the vector, and then so is the result's
    scale, f32(s_a) * f32(s_b[n])."""
    acc = int_matmul(a, b)
    s = np.float32(s_a) * np.asarray(s_b, np.float32)
    s = s if s.ndim else np.float32(s)
    k = a.shape[-1]
    if zp_a is None and zp_b is None:
        return acc, s, None
    row = a.sum(axis=-1, keepdims=True)
    col = b.sum(axis=-2, keepdims=True)
    if zp_a is None:
        return acc, s, row * zp_b
    if zp_b is None:
        return acc, s, col * zp_a
    return acc, s, row * zp_b + col * zp_a - zp_a * zp_b * k


# ----------------------------------------------------------------------------- model level
def calibrate(graph, calibration_inputs, bit_width=8, per_channel=True):
    """Model.quantize(per_channel=...): the oracle's calibration, then every eligible weight
    re-quantized with its column scales and the biases of their Gemms with bscale[n].
    Returns (qparams, qconstants, {name: axis} of the per-column weights)."""
    with np.errstate(all="ignore"):
        qp, qconst = O.calibrate(graph, calibration_inputs, bit_width)
    axes = {}
    if not per_channel:
        return qp, qconst, axes
    cons = consumers(graph)
    for name, arr in graph.constants.items():
        axis = eligible_axis(graph, name, cons)
        if axis is None:
            continue
        s = column_scales(arr, axis, bit_width)
        axes[name] = axis
        qp[name] = O.QParams(s, None)
        qconst[name] = O.Q(quantize_cols(arr, s, bit_width, axis), bit_width, s, None)
    for _, op, _, ins, _ in graph.nodes:
        if op == "Gemm" and ins[1] in axes:
            bscale = (np.float32(qp[ins[0]].scale) * qp[ins[1]].scale).astype(np.float32)
            qp[ins[2]] = O.QParams(bscale, None)
            qconst[ins[2]] = O.Q(quantize_cols(graph.constants[ins[2]], bscale, 4 * bit_width), 4 * bit_width,
                                 bscale, None)
    return qp, qconst, axes


def _deq(t):
    if np.ndim(t[3]) == 1:
        return O.F(dequantize_cols(t[1], t[3], t[4]))
    return O.q_dequant(t)


def quantized_forward(graph, qp, qconst, inputs, bit_width):
    """QModel.__call__ (model.py:486-565) as oracle.quantized_forward runs it, with the MatMul /
    Gemm products through q_matmul above and the vector-aware dequantize / requantize.
    Returns {value: tagged tensor}."""
    vals = dict(qconst)
    for arr, name in zip(inputs, graph.inputs):
        p = qp[name]
        if arr.dtype == np.float32:
            vals[name] = O.Q(O.quantize(arr, bit_width, p.scale, p.zero_point), bit_width, p.scale, p.zero_point)
        else:
            vals[name] = O.I(arr)
    with np.errstate(all="ignore"):
        for _, op, attrs, ins, outs in graph.nodes:
            args = []
            for i in ins:
                t = vals[i]
                if op in ("MatMul", "Gemm") and t[0] == "F":
                    p = qp[i]
                    t = O.Q(O.quantize(t[1], bit_width, p.scale, p.zero_point), bit_width, p.scale, p.zero_point)
                elif op not in ("MatMul", "Gemm") and t[0] == "Q":
                    t = _deq(t)
                args.append(t)
            if op in ("MatMul", "Gemm") and args[0][0] == "Q":
                x, w = args[0], args[1]
                xa, wa = x[1], w[1]
                if op == "Gemm" and attrs.get("transA"):
                    xa = xa.T
                if op == "Gemm" and attrs.get("transB"):
                    wa = wa.T  # the vector of a transB weight lies on axis 0: the last after .T
                assert x[2] == w[2] and np.ndim(x[3]) == 0
                acc, s, z = q_matmul(xa, x[3], x[4], wa, w[3], w[4])
                if op == "Gemm":
                    p = qp[outs[0]]
                    acc = acc + args[2][1]
                    res = [O.Q(requantize_cols(acc, s, z, p.scale, p.zero_point, bit_width), bit_width, p.scale,
                               p.zero_point)]
                else:
                    res = [O.Q(acc, 4 * x[2], s, z)]
            else:
                res = O._float_op(op, args, attrs)
            for o, r in zip(outs, res):
                vals[o] = r
    return vals


def outputs_of(graph, vals):
    return [vals[n][1] if vals[n][0] == "F" else _deq(vals[n])[1] for n in graph.outputs]


# ----------------------------------------------------------------------------- fixtures
def spread_columns(proto, graph, seed, lo=-3.0, hi=3.0):
    """Scale every output column of every eligible weight of `proto` by 2^u, u uniform in
    [lo, hi] and seeded: weights whose columns differ in range, which one scale serves badly."""
    rng = np.random.default_rng(seed)
    cons = consumers(graph)
    count = 0
    for t in proto.graph.initializer:
        axis = eligible_axis(graph, t.name, cons)
        if axis is None:
            continue
        w = graph.constants[t.name]
        f = np.exp2(rng.uniform(lo, hi, size=w.shape[axis])).astype(np.float32)
        t.set_array((w * _along(f, axis)).astype(np.float32))
        count += 1
    return count


def mse(ref, got):
    d = np.asarray(ref, np.float64) - np.asarray(got, np.float64)
    return float(np.mean(d * d))


SEED = 7  # the accuracy fixture's: the restatement's 4-bit output MSE is lower per column (test_perchannel_host)
LAYER = "vit_image_classifier_encoder_layer_no_weights.onnx"


def encoder_layer_fixture(models_dir, seed=SEED, batch=2):
    """(proto, graph, x): the encoder-layer graph with seeded stand-in weights whose columns are
    spread log-uniformly over 2^-3..2^3, and one seeded input batch [batch, 197, 768]."""
    import os
    from numpy_quant import onnx_proto  # the ONNX reader only (oracle.Graph uses it too)
    proto = onnx_proto.load(os.path.join(models_dir, LAYER), synthetic_weights=True, seed=seed)
    if batch != 1:
        onnx_proto.rebatch(proto, batch)
    spread_columns(proto, O.Graph(proto), seed)
    x = np.random.default_rng(seed).standard_normal((batch, 197, 768)).astype(np.float32)
    return proto, O.Graph(proto), x


# ----------------------------------------------------------------------------- fused epilogues
# nqk_qgemm_fused with nqk_epilogue.s_col: tests/_fused_ref.py's chain (q_matmul's zero-point
# algebra, dequantize, the consumer chain, quantize) with the vector in s_acc's place.
# Operands: a [M][K] int8, bt [N][K] int8 (the transposed weight), s_col float32 [N].
def fused_biased(a, bt, zpa, s_col, bias):
    acc = int_matmul(a, bt.T)
    z = bt.astype(np.int64).sum(axis=1)[None, :] * np.int64(zpa)
    return dequantize_cols(acc, s_col, z) + np.asarray(bias, np.float32)


def fused_qkv(a, bt, bias, zpa, s_col, s_out, zp_out, bw, tokens, heads, hdim):
    """NQK_EPI_QKV: three column groups of N / 3, each quantized with its own output parameters
    and head-split ([img, T, H, Dh] -> [img, H, T, Dh] rows; rows past M are zero)."""
    from _fused_ref import head_split
    y = fused_biased(a, bt, zpa, s_col, bias)
    G = bt.shape[0] // 3
    outs = []
    for g in range(3):
        q = O.quantize(y[:, g * G:(g + 1) * G], bw, np.float32(s_out[g]), np.int64(zp_out[g]))
        outs.append(head_split(q.astype(np.int8), a.shape[0], tokens, heads, hdim))
    return outs


def fused_resid(a, bt, bias, res, zpa, s_col):
    """NQK_EPI_RESID: (d + bias) + resid in f32."""
    return fused_biased(a, bt, zpa, s_col, bias) + np.asarray(res, np.float32)


def fused_gelu(a, bt, bias, zpa, s_col, s_out, zp_out, bw):
    """NQK_EPI_GELU with the ViT constants: int64 quantized values [M][N]."""
    from _fused_ref import gelu_values
    y = gelu_values(fused_biased(a, bt, zpa, s_col, bias))
    assert y.dtype == np.float32
    return O.quantize(y, bw, np.float32(s_out), np.int64(zp_out))


# k_pg's QKV rounding filter with per-column constants (nqk_pgemm_kernel.h): an element is decided
# by u = fma(v, c1[n], c2[n]), c1[n] = RN32(s_col[n] rsf[g]), c2[n] = RN32(bias[n] rsf[g]), unless
# |u - rint(u)| + |v| k1[n] reaches the lane's limit; then pg_exact_fix runs the reference chain.
PG_QLIM = np.float32(float.fromhex("0x1.fffffcp-2"))
PG_QK1 = np.float32(float.fromhex("0x1.9p-22"))
PG_QKC2 = np.float32(float.fromhex("0x1.5p-22"))


def qkv_exact_fix_count(a, bt, bias, zpa, s_col, s_out):
    """How many elements of a QKV call take pg_exact_fix (the fma as a float64 sum rounded once
    more: exact for the ties this is used to count)."""
    f32, f64 = np.float32, np.float64
    N = bt.shape[0]
    G = N // 3
    v = int_matmul(a, bt.T) - bt.astype(np.int64).sum(axis=1)[None, :] * np.int64(zpa)
    vf = v.astype(f32)
    rsf = np.repeat(np.array([f32(1.0 / f64(f32(s))) for s in s_out], f32), G)
    c1 = (np.asarray(s_col, f32) * rsf).astype(f32)
    c2 = (np.asarray(bias, f32) * rsf).astype(f32)
    k1 = (np.abs(c1) * PG_QK1).astype(f32)
    u = (vf.astype(f64) * c1.astype(f64) + c2.astype(f64)).astype(f32)
    m = (np.abs(vf).astype(f64) * k1.astype(f64) + np.abs(u - np.rint(u)).astype(f64)).astype(f32)
    cm = np.abs(c2).reshape(-1, 16).max(axis=1)  # a lane's 16 columns share one limit
    lim = np.repeat(((PG_QLIM - cm * PG_QKC2).astype(f32) - f32(2.0 ** -22)).astype(f32), 16)
    return int(np.count_nonzero(~(m < lim[None, :])))
