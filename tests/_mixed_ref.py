"""NumPy restatement of a separate weight bit width (QModel.weight_bit_width): the specification.

The reference quantizes everything at one width (numpy_quant/model.py:338-442).  Here the MatMul /
Gemm weights take a width w of their own, 1 <= w <= bw; every formula is the reference's
(numpy_quantization.py:7-72, restated in oracle/nq_oracle.py), with w in bw's place where a weight
is quantized and nowhere else.  Nothing here imports numpy_quant but its ONNX reader.

Eligible   a 2-D constant each consumer of which is a MatMul taking it as input 1 or a Gemm taking
           it as its weight, input 1 (tests/_perchannel_ref.py eligible_axis: per_channel's rule).
           Conv weights, LayerNorm parameters, position embeddings and activations keep bw.
Weight     s_w, _ = quant_parameters(min W, max W, w, False); q = quantize(W, w, s_w, None);
           per column (per_channel): s_w[n] = column_scales(W, axis, w), q by quantize_cols at w.
q_matmul   unchanged: the integers of a [-2^(bw-1), 2^(bw-1)) activation times a
           [-2^(w-1), 2^(w-1)) weight; the result has width 4 bw and scale f32(s_a) f32(s_w).
           Two operands of which the right one is no weight still need equal widths.
Bias       a Gemm bias at 4 bw with s_x s_w, an Add bias at 4 bw with its input's scale: as before.
Requantize a Gemm output at bw: as before.
"""
import numpy as np

import _fused_ref as F
import _perchannel_ref as P
from oracle import nq_oracle as O


# ----------------------------------------------------------------------------- definition
def weight_width(bit_width, weight_bit_width):
    """w of the rule above: None means bw; anything but an int in 1..bw is a ValueError."""
    if weight_bit_width is None:
        return bit_width
    if isinstance(weight_bit_width, bool) or not isinstance(weight_bit_width, (int, np.integer)) \
            or not 1 <= weight_bit_width <= bit_width:
        raise ValueError(f"weight_bit_width {weight_bit_width!r} is not in 1..{bit_width}")
    return int(weight_bit_width)


def eligible(graph):
    """{name: output-column axis} of the constants that take the weight width."""
    cons = P.consumers(graph)
    out = {}
    for name in graph.constants:
        axis = P.eligible_axis(graph, name, cons)
        if axis is not None:
            out[name] = axis
    return out


def weight_range(arr):
    """The calibrated range of a constant (model.py:329-336: the mean of one minimum / maximum)."""
    flat = arr.reshape((arr.shape[0], -1) if arr.shape else (-1,))
    return np.mean(flat.min()), np.mean(flat.max())


def quantize_weight(arr, w, per_channel=False, axis=1):
    """(integers int64, scale) of an eligible weight at width w."""
    if per_channel:
        s = P.column_scales(arr, axis, w)
        return P.quantize_cols(arr, s, w, axis), s
    mn, mx = weight_range(arr)
    s, _ = O.quant_parameters(mn, mx, w, False)
    return O.quantize(arr, w, s, None), s


# ----------------------------------------------------------------------------- model level
def calibrate(graph, calibration_inputs, bit_width=8, weight_bit_width=None, per_channel=False):
    """Model.quantize(bit_width, weight_bit_width=, per_channel=): the oracle's calibration at
    bit_width, then every eligible weight quantized again at its own width and the biases of their
    Gemms with s_x s_w (4 bit_width).  Returns (qparams, qconstants, {weight name: axis})."""
    w = weight_width(bit_width, weight_bit_width)
    with np.errstate(all="ignore"):
        qp, qconst = O.calibrate(graph, calibration_inputs, bit_width)
    axes = eligible(graph)
    for name, axis in axes.items():
        q, s = quantize_weight(graph.constants[name], w, per_channel, axis)
        qp[name] = O.QParams(s, None)
        qconst[name] = O.Q(q, w, s, None)
    for _, op, _, ins, _ in graph.nodes:
        if op == "Gemm" and ins[1] in axes:
            s_x, s_w = qp[ins[0]].scale, qp[ins[1]].scale
            if np.ndim(s_w) == 1:
                bscale = (np.float32(s_x) * s_w).astype(np.float32)
                qb = P.quantize_cols(graph.constants[ins[2]], bscale, 4 * bit_width)
            else:
                bscale = s_x * s_w
                qb = O.quantize(graph.constants[ins[2]], 4 * bit_width, bscale, None)
            qp[ins[2]] = O.QParams(bscale, None)
            qconst[ins[2]] = O.Q(qb, 4 * bit_width, bscale, None)
    return qp, qconst, axes


def in_range(q, bits):
    lo, hi = O.qrange(bits)
    return q.size == 0 or (q.min() >= lo and q.max() <= hi)


def quantized_forward(graph, qp, qconst, inputs, bit_width, weights=()):
    """QModel.__call__ (model.py:486-565) as oracle.quantized_forward runs it.  `weights`: the names
    that may be narrower than the activation they multiply.  Returns {value: tagged tensor}."""
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
                    t = P._deq(t)
                args.append(t)
            if op in ("MatMul", "Gemm") and args[0][0] == "Q":
                x, w = args[0], args[1]
                xa, wa = x[1], w[1]
                if op == "Gemm" and attrs.get("transA"):
                    xa = xa.T
                if op == "Gemm" and attrs.get("transB"):
                    wa = wa.T
                # the width rule: a weight may be narrower, anything else has the left operand's width
                assert (w[2] <= x[2]) if ins[1] in weights else (w[2] == x[2]), (ins, x[2], w[2])
                assert np.ndim(x[3]) == 0 and in_range(xa, x[2]) and in_range(wa, w[2])
                acc, s, z = P.q_matmul(xa, x[3], x[4], wa, w[3], w[4])
                if op == "Gemm":
                    p = qp[outs[0]]
                    assert args[2][2] == 4 * bit_width
                    acc = acc + args[2][1]
                    if np.ndim(s) == 1:
                        q = P.requantize_cols(acc, s, z, p.scale, p.zero_point, bit_width)
                    else:
                        q = O.requantize(acc, s, z, p.scale, p.zero_point, bit_width)
                    res = [O.Q(q, bit_width, p.scale, p.zero_point)]
                else:
                    res = [O.Q(acc, 4 * x[2], s, z)]
            else:
                res = O._float_op(op, args, attrs)
            for o, r in zip(outs, res):
                vals[o] = r
    return vals


outputs_of = P.outputs_of
mse = P.mse
encoder_layer_fixture = P.encoder_layer_fixture  # tests/test_gpu_perchannel.py's spread stand-in weights


def sqnr_db(ref, got):
    ref = np.asarray(ref, np.float64)
    return float(10.0 * np.log10(np.mean(ref * ref) / mse(ref, got)))


# ----------------------------------------------------------------------------- fused epilogues
# nqk_qgemm_fused with nqk_epilogue.w_bits = w and bit_width = bw: tests/_fused_ref.py's chains (per
# column: tests/_perchannel_ref.py's), which never read a width but the output's; w_bits is a
# statement about bt, checked here.  a [M][K] int8, bt [N][K] int8; `s`: the scalar s_acc (per group
# for QKV) or the float32 vector s_col [N].
def _operands(a, bt, w_bits):
    assert a.dtype == np.int8 and bt.dtype == np.int8 and in_range(bt, w_bits)


def _vec(s):
    return isinstance(s, np.ndarray) and s.ndim == 1 and s.shape[0] > 3


def fused_qkv(a, bt, bias, zpa, s, s_out, zp_out, bw, w_bits, tokens, heads, hdim):
    _operands(a, bt, w_bits)
    if _vec(s):
        return P.fused_qkv(a, bt, bias, zpa, s, s_out, zp_out, bw, tokens, heads, hdim)
    return F.qkv(a, bt, bias, zpa, s, s_out, zp_out, bw, tokens, heads, hdim)


def fused_qkv_values(a, bt, bias, zpa, s, s_out, zp_out, bw, w_bits):
    """The QKV epilogue's value before the clamp, rint(zp + f32(y / s_out)) as float64 [M][N], and the
    distance of zp + y / s_out from a rounding tie: what the tests read the clip and tie counts from."""
    _operands(a, bt, w_bits)
    N = bt.shape[0]
    G = N // 3
    y = P.fused_biased(a, bt, zpa, s, bias) if _vec(s) else \
        np.concatenate([F._biased(a, bt, zpa, s[g], bias, slice(g * G, (g + 1) * G)) for g in range(3)], axis=1)
    so = np.repeat(np.asarray(s_out, np.float32), G)[None, :]
    zo = np.repeat(np.asarray(zp_out, np.float64), G)[None, :]
    u = zo + np.true_divide(y, so).astype(np.float64)
    return np.rint(u), np.abs(u - np.floor(u) - 0.5)


def fused_resid(a, bt, bias, res, zpa, s, w_bits):
    _operands(a, bt, w_bits)
    if _vec(s):
        return P.fused_resid(a, bt, bias, res, zpa, s)
    return F.resid(a, bt, bias, res, zpa, s)


def fused_gelu(a, bt, bias, zpa, s, s_out, zp_out, bw, w_bits):
    """int64 quantized values [M][N]"""
    _operands(a, bt, w_bits)
    if _vec(s):
        return P.fused_gelu(a, bt, bias, zpa, s, s_out, zp_out, bw)
    return F.gelu(a, bt, bias, zpa, s, s_out, zp_out, bw)


def fused_gelu_values(a, bt, bias, zpa, s, s_out, zp_out, w_bits):
    """rint(zp + f32(gelu / s_out)) before the clamp, float64 [M][N]."""
    _operands(a, bt, w_bits)
    h = P.fused_biased(a, bt, zpa, s, bias) if _vec(s) else F._biased(a, bt, zpa, s, bias)
    y = F.gelu_values(h)
    return np.rint(np.float64(zp_out) + np.true_divide(y, np.float32(s_out)).astype(np.float64))


# ----------------------------------------------------------------------------- k_pg's bounds
# k_pg<B4> multiplies the activation bytes by the bytes 16 w on the int8 MFMA, from the initial
# accumulator -16 col[n] zpa.  Every partial sum is bounded by
#   16 (128 sum_k |w[n][k]| + |col[n]| |zpa|) <= 16 (128 col_l1max + col_absmax |zpa|),
# which the launcher requires below 2^31; the f32 epilogues need |acc - col zpa| < 2^24, which
#   128 col_l1max + col_absmax |zpa| < 2^24
# implies (the host's abound + cmax |zpa|).  For w_bits <= 4, |w| <= 8: at K = 3072 and any int8
# zero point both terms are at most 128 * 8 * 3072 = 3145728, 16 * their sum 100663296 < 2^31 and
# their sum 6291456 < 2^24.
def pg_bounds(bt, zpa):
    """(int32 bound, f32 bound) as the launcher computes them from col_l1max and col_absmax."""
    b = bt.astype(np.int64)
    l1max, absmax = int(np.abs(b).sum(axis=1).max()), int(np.abs(b.sum(axis=1)).max())
    inner = 128 * l1max + absmax * abs(int(zpa))
    return 16 * inner, inner


def pg_partial_sums(a, bt, zpa):
    """Per element (m, n): the largest |partial sum| of k_pg<B4>'s accumulator over k (int64
    [M][N]), starting from -16 col[n] zpa and adding 16 a[m][k] bt[n][k] in k order, and the
    final |acc - col zpa| the f32 epilogue converts."""
    a64, b64 = a.astype(np.int64), bt.astype(np.int64)
    start = -16 * b64.sum(axis=1) * np.int64(zpa)                       # [N]
    worst = np.abs(start)[None, :].repeat(a.shape[0], axis=0)
    run = np.broadcast_to(start[None, :], worst.shape).copy()
    for k in range(a.shape[1]):
        run += 16 * a64[:, k:k + 1] * b64[:, k][None, :]
        np.maximum(worst, np.abs(run), out=worst)
    final = run // 16
    assert np.array_equal(final * 16, run)
    return worst, np.abs(final)


def extreme_columns(bt, a, rows=(0, 1)):
    """Put the extremes of §3 into the operands in place: weight columns 0 / 1 all -8 / all 7, column 2
    alternating -8, 7; activation rows `rows` all -128 / all 127 (so -128 and 127 meet -8 and 7 in one column)."""
    bt[0, :] = -8
    bt[1, :] = 7
    bt[2, 0::2] = -8
    bt[2, 1::2] = 7
    a[rows[0], :] = -128
    a[rows[1], :] = 127
