"""GPU parity of the long-sequence one-kernel attention (nqk_attention_long, 225 tokens and up)
with the three-launch chain it replaces (nqk_qgemm_fused SCORES -> nqk_softmax_quant ->
nqk_qgemm_fused PV), which tests/test_gpu_plan.py pins to the eager node loop and the reference.
Integer outputs: bit-exact.  The token counts sit on the kernel's edges: the query-block size (16),
the key-chunk size of the P V product (64), and the depths of NumPy's pairwise row sum (one split up
to 256 elements, two up to 512, three up to 1024, four above)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DH = 64
SENTINEL = 0x5A


def _max_t():
    from numpy_quant import _lib
    return _lib.ATTN_LONG_MAX_T


def _attn(H, T, zq, zk, zp, zv, zc, bw, s_p, s_qk, hdim=DH):
    from numpy_quant import _lib
    s_q, s_k, s_v = np.float32(s_qk[0]), np.float32(s_qk[1]), np.float32(0.043)
    s_p = np.float32(s_p)
    a = _lib.Attention()
    a.heads, a.tokens, a.hdim, a.ld_out, a.bit_width = H, T, hdim, H * hdim, bw
    a.zq, a.zk, a.s_qk, a.div = zq, zk, float(np.float32(s_q * s_k)), 8.0
    a.s_p, a.zp_p, a.s_pv, a.zv = float(s_p), zp, float(np.float32(s_p * s_v)), zv
    a.s_ctx, a.zp_ctx = float(np.float32(0.017)), zc
    return a


def _inputs(B, H, T, bw, seed):
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bw - 1)), (1 << (bw - 1)) - 1
    return [rng.integers(lo, hi + 1, size=(B * H * T, DH), dtype=np.int8) for _ in range(3)]


def _long(dq, dk, dv, B, a, q_rows=0, fill=None):
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    T, D = a.tokens, a.ld_out
    ctx = DeviceArray((B, T, D), np.int8) if fill is None else DeviceArray.from_host(np.full((B, T, D), fill, dtype=np.int8))
    a.q_rows = q_rows
    _lib.call("nqk_attention_long", dq.vp, dk.vp, dv.vp, ctx.vp, B * a.heads, ctypes.byref(a))
    a.q_rows = 0
    return ctx.to_host()


def _chain(dq, dk, dv, B, a):
    """The three launches, with the parameters of `a`."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.plan import EPI_PV, EPI_SCORES, _gemm
    H, T, D, bw = a.heads, a.tokens, a.ld_out, a.bit_width
    Tp = (T + 15) // 16 * 16
    vt = DeviceArray((B * H, DH, Tp), np.int8)
    s = DeviceArray((B * H, T, T), np.float32)
    p = DeviceArray((B * H, T, Tp), np.int8)
    ctx = DeviceArray.from_host(np.full((B, T, D), ~SENTINEL, dtype=np.int8))  # never the other run's bytes
    _lib.call("nqk_transpose_pad_i8", dv.vp, vt.vp, None, B * H, T, DH, Tp)
    e = _lib.Epilogue()
    e.bit_width, e.tokens, e.heads, e.hdim = bw, T, H, DH
    e.group_cols = 1 << 30
    e.zp_flags = _lib.ZP_ROW | _lib.ZP_COL | _lib.ZP_KCONST
    e.zpa, e.zpb, e.kdim = a.zq, a.zk, DH
    e.s_acc[0] = a.s_qk
    e.out[0] = s.ptr
    e.div, e.add1, e.mul2 = a.div, 0.0, 1.0
    _gemm(EPI_SCORES, dq, dk, B * H, T, T, DH, DH, DH, None, T * DH, T * DH, e)
    _lib.call("nqk_softmax_quant", s.vp, p.vp, None, B * H * T, T, Tp, a.s_p, a.zp_p, bw)
    e2 = _lib.Epilogue()
    e2.bit_width, e2.tokens, e2.heads, e2.hdim, e2.ld_out = bw, T, H, DH, D
    e2.group_cols = 1 << 30
    e2.zp_flags = _lib.ZP_ROW | _lib.ZP_COL | _lib.ZP_KCONST
    e2.zpa, e2.zpb, e2.kdim = a.zp_p, a.zv, T
    e2.s_acc[0] = a.s_pv
    e2.s_out[0], e2.zp_out[0], e2.out[0] = a.s_ctx, a.zp_ctx, ctx.ptr
    e2.div, e2.add1, e2.mul2 = 1.0, 0.0, 1.0
    _gemm(EPI_PV, p, vt, B * H, T, DH, Tp, Tp, Tp, None, T * Tp, DH * Tp, e2)
    return ctx.to_host()


def _run_both(B, H, T, zq, zk, zp, zv, zc, bw=8, seed=0, s_p=1.0 / 255, s_qk=(0.031, 0.027)):
    from numpy_quant.device import DeviceArray
    dq, dk, dv = (DeviceArray.from_host(x) for x in _inputs(B, H, T, bw, seed))
    a = _attn(H, T, zq, zk, zp, zv, zc, bw, s_p, s_qk)
    return _long(dq, dk, dv, B, a, fill=SENTINEL), _chain(dq, dk, dv, B, a)


@pytest.mark.parametrize("T", [225, 226, 255, 256, 257, 288, 511, 512, 513, 577, 1025, "max"])
def test_long_attention_matches_three_launch_chain(T):
    T = _max_t() if T == "max" else T
    f, u = _run_both(2, 3, T, zq=-5, zk=3, zp=-128, zv=2, zc=-7, seed=T)
    np.testing.assert_array_equal(f, u)


# (4096, -4096, 1024, -1024): the fixed limits, which the token-dependent bound admits at 577 tokens
# (577 * (16384 + 128 * 2048 + 1024 * 1024) = 7.7e8 < 2^31)
@pytest.mark.parametrize("zq,zk,zp,zv,zc,bw", [(0, 0, 0, 0, 0, 8), (-140, 131, -128, -138, 5, 8),
                                              (4096, -4096, 1024, -1024, 0, 8), (-9, 2, -8, 1, 3, 4)])
def test_long_attention_zero_points_and_bit_widths(zq, zk, zp, zv, zc, bw):
    f, u = _run_both(2, 3, 577, zq, zk, zp, zv, zc, bw=bw, seed=abs(zq) + bw)
    np.testing.assert_array_equal(f, u)


def test_long_attention_four_bits_peaked_rows():
    """At 4 bits and 577 tokens the flat softmax of the case above quantizes every probability to
    the zero point (the context is the constant zp_ctx); larger score scales give peaked rows and a
    context that varies."""
    f, u = _run_both(2, 3, 577, -9, 2, -8, 1, 3, bw=4, seed=44, s_p=1.0 / 15, s_qk=(0.6, 0.7))
    assert len(np.unique(u)) > 2
    np.testing.assert_array_equal(f, u)


@pytest.mark.parametrize("s_p,zp,s_qk", [(8.051e-05, -142, (0.02, 0.0225)), (2.3e-4, -131, (0.011, 0.009)),
                                         (1.0 / 255, -128, (0.002, 0.003))])
def test_long_attention_calibrated_softmax_scales(s_p, zp, s_qk):
    """The calibrated-softmax parameter sets of tests/test_gpu_attention.py: P clamped at the bottom
    (zp < -128) and peaked rows."""
    f, u = _run_both(4, 12, 577, zq=0, zk=-6, zp=zp, zv=-14, zc=-11, seed=int(zp) + 1000, s_p=s_p, s_qk=s_qk)
    np.testing.assert_array_equal(f, u)


@pytest.mark.parametrize("T,q_rows", [(577, 1), (577, 33), (257, 33)])
def test_long_attention_query_row_prefix(T, q_rows):
    from numpy_quant.device import DeviceArray
    B, H = 2, 3
    dq, dk, dv = (DeviceArray.from_host(x) for x in _inputs(B, H, T, 8, T + q_rows))
    a = _attn(H, T, -5, 3, -128, 2, -7, 8, 1.0 / 255, (0.031, 0.027))
    full = _long(dq, dk, dv, B, a, fill=SENTINEL)
    assert (full != SENTINEL).any()
    out = _long(dq, dk, dv, B, a, q_rows=q_rows, fill=SENTINEL)
    np.testing.assert_array_equal(out[:, :q_rows], full[:, :q_rows])
    assert (out[:, q_rows:] == SENTINEL).all(), "a row past the prefix was written"
    np.testing.assert_array_equal(_long(dq, dk, dv, B, a, q_rows=T, fill=SENTINEL), full)


def test_long_attention_per_part_calls():
    """The plan's per-part calls: images [0, 2) and [2, 3) on offset views equal one call over all 3."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    B, H, T = 3, 3, 226
    D = H * DH
    dq, dk, dv = (DeviceArray.from_host(x) for x in _inputs(B, H, T, 8, 5))
    a = _attn(H, T, -5, 3, -128, 2, -7, 8, 1.0 / 255, (0.031, 0.027))
    whole = _long(dq, dk, dv, B, a)
    ctx = DeviceArray.from_host(np.full((B, T, D), SENTINEL, dtype=np.int8))
    for i0, nb in ((0, 2), (2, 1)):
        q, k, v = (x.offset_view(i0 * H * T * DH, (nb * H * T, DH)) for x in (dq, dk, dv))
        c = ctx.offset_view(i0 * T * D, (nb, T, D))
        _lib.call("nqk_attention_long", q.vp, k.vp, v.vp, c.vp, nb * H, ctypes.byref(a))
    np.testing.assert_array_equal(ctx.to_host(), whole)


def _refused(a, T_alloc, null=False):
    """The call is an error.  The buffers hold what the shape asks for, so that a refusal that went
    missing would still launch in bounds."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    H = a.heads
    bufs = [DeviceArray((H * T_alloc, DH), np.int8) for _ in range(4)]
    ptrs = [None] * 4 if null else [b.vp for b in bufs]
    with pytest.raises(_lib.NQKError):
        _lib.call("nqk_attention_long", *ptrs, H, ctypes.byref(a))


def test_long_attention_refusals():
    ok = dict(zq=-5, zk=3, zp=-128, zv=2, zc=-7, bw=8, s_p=1.0 / 255, s_qk=(0.031, 0.027))
    _refused(_attn(1, 224, **ok), 224)                      # nqk_attention_fused's range
    _refused(_attn(1, _max_t() + 1, **ok), _max_t() + 1)    # past the LDS budget
    _refused(_attn(1, 577, hdim=32, **ok), 577)
    _refused(_attn(1, 577, **ok), 577, null=True)
    # the fixed zero-point limits hold, the token-dependent int32 bound does not:
    # 1856 * (16384 + 128 * 2048 + 1024 * 1024) = 2.46e9 >= 2^31
    big = dict(ok, zp=1024, zv=-1024)
    _refused(_attn(1, _max_t(), **big), _max_t())
    a = _attn(1, 577, **ok)
    a.q_rows = 578
    _refused(a, 577)
