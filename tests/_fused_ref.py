"""Plain NumPy restatements of the fused kernels' operations (include/nqk.h nqk_qgemm_fused,
nqk_softmax_quant, nqk_transpose_pad_i8, nqk_attention_fused), built only from the pinned
oracle's primitives (oracle/nq_oracle.py: q_matmul's zero-point algebra, dequantize, quantize,
erf, and _float_op for Softmax / LayerNormalization).  Nothing here imports numpy_quant.

Every function takes host arrays plus the scalars a test puts into nqk_epilogue / nqk_attention
and returns what the kernel must write, bit for bit.  tests/test_fused_ref.py pins each of them
to the oracle's node loop on the encoder-layer graph (CPU only).

Operands: a [M][K] int8, bt [N][K] int8 (the transposed weight, as the kernels take it)."""
import numpy as np

from oracle import nq_oracle as O

SQRT2_F32 = np.float32(1.4142135381698608)
_checked = set()


def int_matmul(a, b):
    """The exact integer product a @ b (last two axes) through float64 BLAS: int8 operands
    give |acc| <= 2^14 K < 2^53, so every partial sum is exact in f64.  The first use of each
    shape class checks one small slice against NumPy's int64 matmul."""
    acc = np.matmul(a.astype(np.float64), b.astype(np.float64)).astype(np.int64)
    key = (a.shape[-1], a.ndim)
    if key not in _checked:
        _checked.add(key)
        sa, sb = a[..., :5, :], b[..., :, :7]
        assert np.array_equal(acc[..., :5, :7], np.matmul(sa.astype(np.int64), sb.astype(np.int64)))
    return acc


def _col_acc(a, bt, zpa):
    """(acc, zero-point term) of q_matmul with an asymmetric A and symmetric weights
    (numpy_quantization.py:44-61, zp_b None): colsum(B) * zp_a, shape (1, N)."""
    acc = int_matmul(a, bt.T)
    col = bt.astype(np.int64).sum(axis=1)[None, :]
    if a.shape[0] >= 1:  # the oracle's own q_matmul on one row: same product, same term
        o_acc, _, o_z = O.q_matmul(a[:1].astype(np.int64), 1.0, np.int64(zpa), bt.T.astype(np.int64), 1.0, None)
        assert np.array_equal(o_acc, acc[:1]) and np.array_equal(o_z, col * np.int64(zpa))
    return acc, col * np.int64(zpa)


def _biased(a, bt, zpa, s_acc, bias, cols=slice(None)):
    acc, z = _col_acc(a, bt[cols], zpa)
    return O.dequantize(acc, np.float32(s_acc), z) + np.asarray(bias, np.float32)[cols]


def head_split(q, M, tokens, heads, hdim):
    """[img, T, H, Dh] -> [img, H, T, Dh] as int8 rows [img * H * T][Dh]; rows past M in the
    last image are zero."""
    nimg = -(-M // tokens)
    full = np.zeros((nimg * tokens, heads * hdim), np.int8)
    full[:M] = q
    return np.ascontiguousarray(full.reshape(nimg, tokens, heads, hdim).transpose(0, 2, 1, 3)).reshape(-1, hdim)


def qkv(a, bt, bias, zpa, s_acc, s_out, zp_out, bw, tokens, heads, hdim, split=True):
    """NQK_EPI_QKV: three column groups of N / 3; returns the three int8 outputs (head-split
    unless split=False: then the [M][N / 3] quantized values as int64)."""
    N = bt.shape[0]
    G = N // 3
    outs = []
    for g in range(3):
        y = _biased(a, bt, zpa, s_acc[g], bias, slice(g * G, (g + 1) * G))
        q = O.quantize(y, bw, np.float32(s_out[g]), np.int64(zp_out[g]))
        outs.append(head_split(q.astype(np.int8), a.shape[0], tokens, heads, hdim) if split else q)
    return outs


def resid(a, bt, bias, res, zpa, s_acc):
    """NQK_EPI_RESID: (d + bias) + resid in f32."""
    return _biased(a, bt, zpa, s_acc, bias) + np.asarray(res, np.float32)


def resid_ln(a, bt, bias, res, zpa, s_acc, gamma, beta, eps, ln_scale, ln_zp, bw):
    """NQK_EPI_RESID with the fused LayerNormalization: (f32 rows, int8 LN output)."""
    y = resid(a, bt, bias, res, zpa, s_acc)
    ln = O._float_op("LayerNormalization", [O.F(y), O.F(np.asarray(gamma, np.float32)), O.F(np.asarray(beta, np.float32))],
                     {"axis": -1, "epsilon": eps})[0][1]
    return y, O.quantize(ln, bw, np.float32(ln_scale), np.int64(ln_zp)).astype(np.int8)


def gelu_values(h, div=SQRT2_F32, add1=1.0, mul2=0.5):
    h = np.asarray(h, np.float32)
    return (h * (O.erf(h / np.float32(div)) + np.float32(add1))) * np.float32(mul2)


def gelu(a, bt, bias, zpa, s_acc, s_out, zp_out, bw, div=SQRT2_F32, add1=1.0, mul2=0.5):
    """NQK_EPI_GELU: int64 quantized values [M][N]."""
    y = gelu_values(_biased(a, bt, zpa, s_acc, bias), div, add1, mul2)
    assert y.dtype == np.float32
    return O.quantize(y, bw, np.float32(s_out), np.int64(zp_out))


def _full_acc(a, b, zpa, zpb, kdim):
    """q_matmul with both operands asymmetric: a [..., M, K], b [..., K, N]."""
    acc = int_matmul(a, b)
    row = a.astype(np.int64).sum(axis=-1, keepdims=True)
    col = b.astype(np.int64).sum(axis=-2, keepdims=True)
    return acc, row * np.int64(zpb) + col * np.int64(zpa) - np.int64(zpa) * np.int64(zpb) * np.int64(kdim)


def scores(q, k, zq, zk, s_qk, div):
    """NQK_EPI_SCORES: q, k [bh][T][Dh] int8 -> f32 [bh][T][T]."""
    acc, z = _full_acc(q, np.swapaxes(k, -1, -2), zq, zk, q.shape[-1])
    return O.dequantize(acc, np.float32(s_qk), z) / np.float32(div)


def softmax_quant(x, ldo, s_p, zp_p, bw):
    """nqk_softmax_quant: (int8 [..., rows, ldo] zero padded, int64 row sums)."""
    p = O._float_op("Softmax", [O.F(np.asarray(x, np.float32))], {"axis": -1})[0][1]
    qv = O.quantize(p, bw, np.float32(s_p), np.int64(zp_p))
    out = np.zeros(x.shape[:-1] + (ldo,), np.int8)
    out[..., :x.shape[-1]] = qv
    return out, qv.sum(axis=-1)


def transpose_pad(src, Rp):
    """nqk_transpose_pad_i8: [nb][R][C] -> ([nb][C][Rp] zero padded, int64 sums over R [nb][C])."""
    nb, R, C = src.shape
    out = np.zeros((nb, C, Rp), np.int8)
    out[:, :, :R] = src.transpose(0, 2, 1)
    return out, src.astype(np.int64).sum(axis=1)


def pv(p, v, zp_p, zv, s_pv, s_ctx, zp_ctx, bw, heads, tokens, ld_out=None):
    """NQK_EPI_PV: p [bh][T][Tp] int8 (columns past T zero), v [bh][T][Dh] int8 ->
    int8 [bh / heads][T][ld_out], head h at columns h * Dh."""
    T, Dh = tokens, v.shape[-1]
    acc, z = _full_acc(p[..., :T], v, zp_p, zv, T)
    qv = O.quantize(O.dequantize(acc, np.float32(s_pv), z), bw, np.float32(s_ctx), np.int64(zp_ctx))
    B = p.shape[0] // heads
    ld = heads * Dh if ld_out is None else ld_out
    out = np.zeros((B, T, ld), np.int8)
    out[:, :, :heads * Dh] = qv.reshape(B, heads, T, Dh).transpose(0, 2, 1, 3).reshape(B, T, heads * Dh)
    return out


def attention(q, k, v, heads, zq, zk, s_qk, div, s_p, zp_p, s_pv, zv, s_ctx, zp_ctx, bw, want_scores=False):
    """nqk_attention_fused: SCORES -> softmax_quant -> PV of the functions above."""
    T = q.shape[1]
    s = scores(q, k, zq, zk, s_qk, div)
    p, _ = softmax_quant(s, (T + 15) // 16 * 16, s_p, zp_p, bw)
    ctx = pv(p, v, zp_p, zv, s_pv, s_ctx, zp_ctx, bw, heads, T)
    return (ctx, s, p) if want_scores else ctx
