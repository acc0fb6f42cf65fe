"""Device-side setup of one nqk_qgemm_fused projection call from host operands, shared by
tests/test_gpu_pgemm.py, tests/test_gpu_glut.py and tests/test_gpu_fused_reference.py: uploads,
the weight images (row-major, nqk_pack_b, nqk_pack_b4, nqk_pack_pg, nqk_pack_pg4), the epilogue
struct, zero-filled outputs, the launch, and the kernel id it took.  And of the attention calls
(tests/test_gpu_fused_reference.py below 225 tokens, tests/test_gpu_attention_long_reference.py
from there on): the nqk_attention struct of a case, and the three-launch chain stage by stage."""
import ctypes

import numpy as np

import _fused_cases as F

SQRT2_F32 = float(np.float32(1.4142135381698608))


def build_gelu_lut(s_out, zp, bw=8):
    """(table, bucket coordinate, entries) of nqk_gelu_lut_build for the GELU of model.py."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    lut = DeviceArray((_lib.load().nqk_gelu_lut_capacity(),), np.uint8)
    k = (ctypes.c_float * 5)()
    n = ctypes.c_int32(-1)
    _lib.call("nqk_gelu_lut_build", float(np.float32(s_out)), int(zp), bw, SQRT2_F32, 1.0, 0.5, lut.vp, k, ctypes.byref(n))
    return lut, k, n.value


def fused_gemm(epi_name, a_h, bt_h, *, zpa, bias_h, s_acc, s_out=(1.0, 1.0, 1.0), zp_out=(0, 0, 0), bw=8, resid_h=None,
               weights="plain", pg=None, use_pg=True, use_col=True, col_l1max=0, tokens=197, ln=None, lut=None):
    """Runs C = A . Bt^T with the epilogue `epi_name` ("qkv", "resid", "gelu").

    weights: "plain" (row-major Bt), "pack" (nqk_pack_b) or "pack4" (nqk_pack_b4).
    pg: None, "pg" (nqk_pack_pg) or "pg4" (nqk_pack_pg4); the image is always built, and offered to
        the launcher (nqk_epilogue.bt_pg) when use_pg.
    use_col: precomputed column sums and col_absmax (without them the small-tile kernel runs).
    The int32 column term col * zpa is passed whenever it exists (|col * zpa| < 2^31).
    ln: dict(gamma, beta, eps, scale, zp) for the fused LayerNorm (a second, int8 output).
    lut: (table, coordinate, entries) of build_gelu_lut.
    Returns (nqk_qgemm_last_kernel(), [outputs on the host], the epilogue struct)."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.plan import EPI_GELU, EPI_QKV, EPI_RESID, _gemm, _pack_b, _pack_pg
    epi = {"qkv": EPI_QKV, "resid": EPI_RESID, "gelu": EPI_GELU}[epi_name]
    (M, K), N = a_h.shape, bt_h.shape[0]
    a, bt = DeviceArray.from_host(np.ascontiguousarray(a_h)), DeviceArray.from_host(np.ascontiguousarray(bt_h))
    keep = [a, bt]

    def up(x):
        keep.append(DeviceArray.from_host(np.ascontiguousarray(x)))
        return keep[-1]

    col_h = bt_h.astype(np.int64).sum(axis=1)
    e = _lib.Epilogue()
    e.zp_flags, e.bit_width, e.zpa = _lib.ZP_COL, bw, zpa
    if use_col:
        e.col, e.col_absmax, e.col_l1max = up(col_h).ptr, int(np.abs(col_h).max()), col_l1max
    e.bias = up(bias_h).ptr
    if np.abs(col_h * zpa).max() < 2 ** 31:
        e.colterm = up((col_h * zpa).astype(np.int32)).ptr
    b_op = bt
    if weights != "plain":
        b_op, kind = _pack_b(bt, 4 if weights == "pack4" else 8)
        assert kind == (2 if weights == "pack4" else 1)
        e.b_packed = kind
        keep.append(b_op)
    if pg:
        image = _pack_pg(bt, 4 if pg == "pg4" else 8, 1 if epi == EPI_RESID else 0, nibbles=pg == "pg4")
        assert image is not None
        keep.append(image)
        e.bt_pg = image.ptr if use_pg else None
    if epi == EPI_QKV:
        H = N // 3 // 64
        e.group_cols, e.tokens, e.heads, e.hdim = N // 3, tokens, H, 64
        bufs = [DeviceArray((-(-M // tokens) * H * tokens, 64), np.int8) for _ in range(3)]
        for g in range(3):
            e.s_acc[g], e.s_out[g], e.zp_out[g], e.out[g] = float(s_acc[g]), float(s_out[g]), int(zp_out[g]), bufs[g].ptr
    elif epi == EPI_RESID:
        e.group_cols = 1 << 30
        bufs = [DeviceArray((M, N), np.float32)]
        e.s_acc[0], e.out[0], e.resid = float(s_acc[0]), bufs[0].ptr, up(resid_h).ptr
        if ln is not None:
            bufs.append(DeviceArray((M, N), np.int8))
            e.ln_gamma, e.ln_beta, e.ln_out = up(ln["gamma"]).ptr, up(ln["beta"]).ptr, bufs[1].ptr
            e.ln_eps, e.ln_scale, e.ln_zp = float(ln["eps"]), float(ln["scale"]), int(ln["zp"])
    else:
        e.group_cols = 1 << 30
        bufs = [DeviceArray((M, N), np.int8)]
        e.s_acc[0], e.s_out[0], e.zp_out[0], e.out[0] = float(s_acc[0]), float(s_out[0]), int(zp_out[0]), bufs[0].ptr
        e.div, e.add1, e.mul2 = SQRT2_F32, 1.0, 0.5
        if lut is not None:
            keep.append(lut[0])
            e.gelu_lut, e.lut_n = lut[0].ptr, lut[2]
            for j in range(5):
                e.lut_k[j] = lut[1][j]
    for b in bufs:
        b.fill_zero()
    _gemm(epi, a, b_op, 1, M, N, K, K, K, None, 0, 0, e)
    kernel = _lib.load().nqk_qgemm_last_kernel()
    outs = [b.to_host() for b in bufs]
    del keep
    return kernel, outs, e


# ------------------------------------------------------------------------------- attention
def attn_params(d, heads, T, bw):
    """The nqk_attention struct of an attention case (tests/_fused_cases.py attn_case / attn_exact_case)."""
    from numpy_quant import _lib
    a = _lib.Attention()
    a.heads, a.tokens, a.hdim, a.ld_out, a.bit_width = heads, T, F.DH, heads * F.DH, bw
    a.zq, a.zk, a.s_qk, a.div = d["zq"], d["zk"], float(d["s_qk"]), d["div"]
    a.s_p, a.zp_p, a.s_pv, a.zv = float(d["s_p"]), d["zp_p"], float(d["s_pv"]), d["zv"]
    a.s_ctx, a.zp_ctx = float(d["s_ctx"]), d["zp_ctx"]
    return a


def head_mismatches(got, want, T):
    """Mismatch counts of a context [B][T][H * Dh] per (image, head)."""
    g, w = (x.reshape(F.B_ATT, T, F.H_ATT, F.DH) for x in (got, want))
    return [int((g[b, :, h] != w[b, :, h]).sum()) for b in range(F.B_ATT) for h in range(F.H_ATT)]


def pv_gemm(d, p_h, vt_h, T, Tp, bw):
    """EPI_PV of the case's parameters on host P [BH][T][Tp] and V^T [BH][Dh][Tp]; the context on the host."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.plan import EPI_PV, _gemm
    BH, Dh, H = F.B_ATT * F.H_ATT, F.DH, F.H_ATT
    p, vt = DeviceArray.from_host(np.ascontiguousarray(p_h)), DeviceArray.from_host(np.ascontiguousarray(vt_h))
    ctx = DeviceArray((F.B_ATT, T, H * Dh), np.int8)
    ctx.fill_zero()
    e = _lib.Epilogue()
    e.bit_width, e.tokens, e.heads, e.hdim, e.ld_out, e.group_cols = bw, T, H, Dh, H * Dh, 1 << 30
    e.zp_flags = _lib.ZP_ROW | _lib.ZP_COL | _lib.ZP_KCONST
    e.zpa, e.zpb, e.kdim = d["zp_p"], d["zv"], T
    e.s_acc[0], e.s_out[0], e.zp_out[0], e.out[0] = float(d["s_pv"]), float(d["s_ctx"]), d["zp_ctx"], ctx.ptr
    e.div, e.add1, e.mul2 = 1.0, 0.0, 1.0
    _gemm(EPI_PV, p, vt, BH, T, Dh, Tp, Tp, Tp, None, T * Tp, Dh * Tp, e)
    assert _lib.load().nqk_qgemm_last_kernel() == 0
    return ctx.to_host()


def check_three_launch_pieces(case):
    """The SCORES and PV epilogues (k_qgemm_epi, batched, row / column / K-constant zero-point
    terms), nqk_softmax_quant and nqk_transpose_pad_i8 with their int64 sums, each fed with the
    reference's own input of that stage and compared with the reference's output of it."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.plan import EPI_SCORES, _gemm
    d = F.attn_case(case)
    T, BH, Dh, H, bw = case.T, F.B_ATT * F.H_ATT, F.DH, F.H_ATT, case.bw
    Tp = (T + 15) // 16 * 16
    dq, dk, dv = (DeviceArray.from_host(d[x].reshape(BH * T, Dh)) for x in "qkv")
    # transpose + pad of V, with the sums over T
    vt, vsum = DeviceArray((BH, Dh, Tp), np.int8), DeviceArray((BH, Dh), np.int64)
    _lib.call("nqk_transpose_pad_i8", dv.vp, vt.vp, vsum.vp, BH, T, Dh, Tp)
    np.testing.assert_array_equal(vt.to_host(), d["vt"])
    np.testing.assert_array_equal(vsum.to_host(), d["vsum"])
    # scores
    s = DeviceArray((BH, T, T), np.float32)
    e = _lib.Epilogue()
    e.bit_width, e.tokens, e.heads, e.hdim, e.group_cols = bw, T, H, Dh, 1 << 30
    e.zp_flags = _lib.ZP_ROW | _lib.ZP_COL | _lib.ZP_KCONST
    e.zpa, e.zpb, e.kdim = d["zq"], d["zk"], Dh
    e.s_acc[0], e.out[0] = float(d["s_qk"]), s.ptr
    e.div, e.add1, e.mul2 = d["div"], 0.0, 1.0
    _gemm(EPI_SCORES, dq, dk, BH, T, T, Dh, Dh, Dh, None, T * Dh, T * Dh, e)
    assert _lib.load().nqk_qgemm_last_kernel() == 0
    np.testing.assert_array_equal(s.to_host().view(np.int32), d["scores"].view(np.int32))
    # softmax + quantize of the reference's scores
    sr = DeviceArray.from_host(np.ascontiguousarray(d["scores"]))
    p, psum = DeviceArray((BH, T, Tp), np.int8), DeviceArray((BH, T), np.int64)
    p.fill_zero()
    _lib.call("nqk_softmax_quant", sr.vp, p.vp, psum.vp, BH * T, T, Tp, float(d["s_p"]), d["zp_p"], bw)
    np.testing.assert_array_equal(p.to_host(), d["p"])
    np.testing.assert_array_equal(psum.to_host(), d["psum"])
    # P . V on the reference's P and V^T
    ctx = pv_gemm(d, d["p"], d["vt"], T, Tp, bw)
    np.testing.assert_array_equal(ctx, d["ctx"])
