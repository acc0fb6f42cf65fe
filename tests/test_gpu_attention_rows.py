"""nqk_attention_fused on a prefix of the query rows (nqk_attention.q_rows): rows below q_rows get
the bytes of the full call, the rows from q_rows on are not written, q_rows = tokens is the full
call, and a q_rows outside [0, tokens] is refused.  Both T = 197 kernels (k_attn16, k_attention),
the non-FAST kernel (a Div that is no power of two), another token count, bit widths 8 and 4, and
parameters that send many elements through the exact fallbacks."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
B, H, DH = 2, 3, 64

# name: (T, NQK_ATTN16, div, bit width, (zq, zk, zp_p, zv, zp_ctx), s_p, (s_q, s_k), s_ctx / s_pv or None)
CASES = {
    "attn16": (197, "1", 8.0, 8, (-5, 3, -128, 2, -7), 1.0 / 255, (0.031, 0.027), None),
    "k_attention": (197, "0", 8.0, 8, (-5, 3, -128, 2, -7), 1.0 / 255, (0.031, 0.027), None),
    "not_fast": (197, "1", 7.0, 8, (-5, 3, -128, 2, -7), 1.0 / 255, (0.031, 0.027), None),
    "t50": (50, "1", 8.0, 8, (4, -2, -128, 1, 3), 1.0 / 255, (0.031, 0.027), None),
    "attn16_bw4": (197, "1", 8.0, 4, (-9, 2, -8, 1, 3), 1.0 / 15, (0.031, 0.027), None),
    "k_attention_bw4": (197, "0", 8.0, 4, (-9, 2, -8, 1, 3), 1.0 / 15, (0.031, 0.027), None),
    # a calibrated softmax scale (the P quantize clamps at the bottom, the filter margins scale with
    # the values) and s_ctx = 2 s_pv: every odd context integer sits exactly on a rounding boundary,
    # so the exact P and context fallbacks run
    "attn16_boundaries": (197, "1", 8.0, 8, (0, -6, -142, -14, -11), 8.051e-05, (0.02, 0.0225), 2.0),
    "k_attention_boundaries": (197, "0", 8.0, 8, (0, -6, -142, -14, -11), 8.051e-05, (0.02, 0.0225), 2.0),
}


def _params(case):
    from numpy_quant import _lib
    T, _, div, bw, (zq, zk, zp, zv, zc), s_p, s_qk, ctx_ratio = CASES[case]
    s_q, s_k, s_v, s_p = np.float32(s_qk[0]), np.float32(s_qk[1]), np.float32(0.043), np.float32(s_p)
    s_pv = np.float32(s_p * s_v)
    s_ctx = np.float32(0.017) if ctx_ratio is None else np.float32(s_pv * np.float32(ctx_ratio))
    a = _lib.Attention()
    a.heads, a.tokens, a.hdim, a.ld_out, a.bit_width = H, T, DH, H * DH, bw
    a.zq, a.zk, a.s_qk, a.div = zq, zk, float(np.float32(s_q * s_k)), div
    a.s_p, a.zp_p, a.s_pv, a.zv = float(s_p), zp, float(s_pv), zv
    a.s_ctx, a.zp_ctx = float(s_ctx), zc
    return a


def _inputs(case):
    from numpy_quant.device import DeviceArray
    T, bw = CASES[case][0], CASES[case][3]
    rng = np.random.default_rng(sorted(CASES).index(case))
    lo, hi = -(1 << (bw - 1)), (1 << (bw - 1)) - 1
    return [DeviceArray.from_host(rng.integers(lo, hi + 1, size=(B * H * T, DH), dtype=np.int8)) for _ in range(3)]


def _run(case, qkv, q_rows):
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    T = CASES[case][0]
    ctx = DeviceArray.from_host(np.full((B, T, H * DH), SENTINEL, dtype=np.int8))
    a = _params(case)
    a.q_rows = q_rows
    _lib.call("nqk_attention_fused", qkv[0].vp, qkv[1].vp, qkv[2].vp, ctx.vp, B * H, ctypes.byref(a))
    return ctx.to_host()


@pytest.mark.parametrize("case", sorted(CASES))
def test_query_row_prefix(case, monkeypatch):
    T = CASES[case][0]
    monkeypatch.setenv("NQK_ATTN16", CASES[case][1])
    monkeypatch.setenv("NQK_ATTN16_NW", "4")
    qkv = _inputs(case)
    full = _run(case, qkv, 0)
    assert (full != SENTINEL).any()
    for q_rows in (1, 5, 16, 17, T):
        out = _run(case, qkv, q_rows)
        np.testing.assert_array_equal(out[:, :q_rows], full[:, :q_rows], err_msg=f"q_rows {q_rows}: computed rows")
        assert (out[:, q_rows:] == SENTINEL).all(), f"q_rows {q_rows}: a row past the prefix was written"
    np.testing.assert_array_equal(_run(case, qkv, T), full)


def test_query_row_prefix_five_waves(monkeypatch):
    """k_attn16 with five waves per workgroup (NQK_ATTN16_NW=5)."""
    monkeypatch.setenv("NQK_ATTN16", "1")
    monkeypatch.setenv("NQK_ATTN16_NW", "5")
    qkv = _inputs("attn16")
    full = _run("attn16", qkv, 0)
    for q_rows in (1, 17, 81):
        out = _run("attn16", qkv, q_rows)
        np.testing.assert_array_equal(out[:, :q_rows], full[:, :q_rows])
        assert (out[:, q_rows:] == SENTINEL).all()


@pytest.mark.parametrize("q_rows", [-1, 198])
def test_bad_q_rows_is_refused(q_rows):
    from numpy_quant import _lib
    a = _params("attn16")
    a.q_rows = q_rows
    qkv = _inputs("attn16")
    from numpy_quant.device import DeviceArray
    ctx = DeviceArray((B, 197, H * DH), np.int8)
    with pytest.raises(_lib.NQKError):
        _lib.call("nqk_attention_fused", qkv[0].vp, qkv[1].vp, qkv[2].vp, ctx.vp, B * H, ctypes.byref(a))
