"""A separate weight bit width (QModel.weight_bit_width, nqk_epilogue.w_bits) on the GPU against the
NumPy restatement (tests/_mixed_ref.py), bit for bit: the products, the fused GEMMs on k_pg's nibble
instances under 8-bit activations and on the kernels that take the call where k_pg declines, the
encoder layer (node loop, plan, graph replay, blob), the classifiers, and the error report."""
import functools
import os

import numpy as np
import pytest

from conftest import ROOT

import _mixed_ref as R
import _perchannel_ref as P
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
SQRT2_F32 = float(np.float32(1.4142135381698608))
PG_BM = 128  # nqk_pgemm_kernel.h: k_pg's tile rows


def _dev(a):
    from numpy_quant.device import DeviceArray
    return DeviceArray.from_host(np.ascontiguousarray(a))


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and
                                         np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))


# ----------------------------------------------------------------------------- 1. products
@pytest.mark.parametrize("shape,route", [((37, 80, 50), "mfma"), ((37, 77, 50), "mfma"), ((5, 16, 7), "generic")],
                         ids=["mfma", "mfma-padded-K", "generic"])
@pytest.mark.parametrize("wbits", [4, 3, 2])
def test_matmul_of_an_8_bit_activation_with_a_narrower_weight(shape, route, wbits):
    from numpy_quant.tensor import FTensor, quantize_tensor
    M, K, N = shape
    rng = np.random.default_rng(100 * wbits + K)
    xf = rng.standard_normal((M, K)).astype(np.float32)
    wf = rng.standard_normal((K, N)).astype(np.float32)
    wf[0, 0] = np.float32(-1.5) * wf.max()  # past the symmetric range's low end: both ends of the width are reached
    s_x, zp_x = O.quant_parameters(xf.min(), xf.max(), 8, True)
    s_w, _ = O.quant_parameters(*R.weight_range(wf), wbits, False)
    xq, wq = O.quantize(xf, 8, s_x, zp_x), O.quantize(wf, wbits, s_w, None)
    assert xq.min() == -128 and xq.max() == 127 and wq.min() == -(1 << (wbits - 1)) and wq.max() == (1 << (wbits - 1)) - 1
    acc, s, z = O.q_matmul(xq, s_x, zp_x, wq, s_w, None)
    x = quantize_tensor(FTensor(xf), 8, s_x, zp_x)
    w = quantize_tensor(FTensor(wf), wbits, s_w, None)
    assert np.array_equal(x.data, xq) and np.array_equal(w.data, wq) and w.bit_width == wbits
    with pytest.raises(AssertionError):
        x.matmul(w)  # not marked as a weight: two tensors of different widths
    w._is_weight = True
    out = x.matmul(w)
    assert out.bit_width == 32
    assert out.dev.dtype == (np.int32 if route == "mfma" else np.int64)  # nqk_qgemm_i8 / nqk_qgemm_generic
    assert np.array_equal(out.data, acc)
    assert np.array_equal(np.asarray(out.scale, np.float32).view(np.uint32), np.asarray(s, np.float32).view(np.uint32))
    assert np.array_equal(np.broadcast_to(out.zero_point, acc.shape), np.broadcast_to(z, acc.shape))
    assert np.array_equal(out.dequantize().data.view(np.uint32), O.dequantize(acc, s, z).view(np.uint32))
    if wbits > 2:  # a weight wider than the activation it multiplies is refused
        x2 = quantize_tensor(FTensor(xf), 2, s_x, zp_x)
        with pytest.raises(AssertionError):
            x2.matmul(w)


def test_two_activations_of_different_widths_and_bad_widths_are_refused():
    from numpy_quant.model import Model
    from numpy_quant.tensor import FTensor, quantize_tensor
    rng = np.random.default_rng(0)
    a = quantize_tensor(FTensor(rng.standard_normal((6, 16)).astype(np.float32)), 8, np.float32(0.03), np.int64(2))
    b = quantize_tensor(FTensor(rng.standard_normal((16, 5)).astype(np.float32)), 4, np.float32(0.4), np.int64(1))
    with pytest.raises(AssertionError):
        a.matmul(b)
    model = Model.from_onnx(os.path.join(MODELS, "mlp.onnx"))
    x = rng.uniform(-1.2, 1.2, size=(8, 2)).astype(np.float32)
    for bad in (0, -4, 9, 4.0, "4", True):
        with pytest.raises(ValueError, match="weight_bit_width"):
            model.quantize([x], bit_width=8, weight_bit_width=bad)
    with pytest.raises(ValueError, match="weight_bit_width"):
        model.quantize_stream([[x]], bit_width=4, weight_bit_width=8)
    assert model.quantize([x], bit_width=8).weight_bit_width == 8
    assert model.quantize([x], bit_width=8, weight_bit_width=np.int64(3)).weight_bit_width == 3


# ----------------------------------------------------------------------------- nqk_qgemm_fused with w_bits
def _fused(epi_name, a_h, bt_h, *, zpa, bias_h, s_acc, s_col=None, s_out=(1.0, 1.0, 1.0), zp_out=(0, 0, 0), bw=8,
           w_bits=4, resid_h=None, tokens=16, pg=True, lut=None, stated=None):
    """One nqk_qgemm_fused call with nibble weights under `bw`-bit activations: bt_pg the nqk_pack_pg4
    image (b_packed = 2), bt the nqk_pack_b4 image, or with s_col the unpacked weight; w_bits stated.
    `stated`: another w_bits for the struct than the images were packed for.  Returns (kernel id, outputs)."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.plan import EPI_GELU, EPI_QKV, EPI_RESID, _gemm, _pack_b, _pack_pg
    epi = {"qkv": EPI_QKV, "resid": EPI_RESID, "gelu": EPI_GELU}[epi_name]
    (M, K), N = a_h.shape, bt_h.shape[0]
    keep = []

    def up(x):
        keep.append(_dev(x))
        return keep[-1]

    a, bt = up(a_h), up(bt_h)
    e = _lib.Epilogue()
    e.zp_flags, e.bit_width, e.zpa, e.w_bits = _lib.ZP_COL, bw, zpa, w_bits if stated is None else stated
    col_h = bt_h.astype(np.int64).sum(axis=1)
    e.col, e.col_absmax = up(col_h).ptr, max(1, int(np.abs(col_h).max()))
    e.col_l1max = max(1, int(np.abs(bt_h.astype(np.int64)).sum(axis=1).max()))
    assert np.abs(col_h * zpa).max() < 2 ** 31
    e.colterm = up((col_h * zpa).astype(np.int32)).ptr
    e.bias = up(bias_h).ptr
    b_op = bt
    e.b_packed = 2
    if s_col is not None:
        e.s_col = up(np.asarray(s_col, np.float32)).ptr
    else:
        b_op, kind = _pack_b(bt, w_bits)
        assert kind == 2
        keep.append(b_op)
    if pg:
        image = _pack_pg(bt, w_bits, 1 if epi == EPI_RESID else 0, nibbles=True)
        if image is not None:
            keep.append(image)
            e.bt_pg = image.ptr
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
    return kernel, outs


@functools.lru_cache(maxsize=None)
def _lut(s_out, zp, bw=8):
    from _fused_gpu import build_gelu_lut
    return build_gelu_lut(s_out, zp, bw)


# GELU outputs: (s_out, zp_out) with about a tenth of the values past each clip bound for
# h ~ N(0, sigma_h).  The chain's minimum is -0.17, so the lower bound is reached only with
# zp + (-0.16 / s_out) < -128.5.  "table": a table of at most 512 entries exists (k_pg<PG_GLUT>);
# "chain": the scale's table needs more than 512 entries, which no nibble instance holds (the
# 256 x 256-tile form has none), so the launcher must drop the table and run the filtered chain.
GELU_OUT = {"table": (float(2.0 ** -7), -108, 1.5), "chain": (0.0027, -70, 0.7)}
CLIP_LO, CLIP_HI = 0.02, 0.25  # "about a tenth": each side's share of the values past the bound


def _case(epi, M, N, K, zpa, pc, gelu="table", w_bits=4, seed=0, tokens=16):
    """Operands, parameters and the restatement's outputs of one call.  Weight columns 0 / 1 / 2 all -8 /
    all 7 / alternating, activation rows 0 / 1 all -128 / all 127 (narrower w_bits: the range's own
    ends).  QKV: power-of-two scales, s_out = 2^k s_acc, biases whole multiples of s_acc: exact ties."""
    rng = np.random.default_rng(9000 + 13 * M + N + K + 7 * zpa + (1 if pc else 0) + seed)
    lo, hi = -(1 << (w_bits - 1)), (1 << (w_bits - 1)) - 1
    a = np.clip(np.rint(rng.standard_normal((M, K)) * 50.0), -128, 127).astype(np.int8)
    # (symmetric, so that sum_k (a - zpa) w has no offset that grows with |zpa|; rows 0 and 2 hold the range's low end)
    bt = rng.integers(lo + 1, hi + 1, size=(N, K)).astype(np.int8)
    a[0, :], a[1, :] = -128, 127
    bt[0, :], bt[1, :] = lo, hi
    bt[2, 0::2], bt[2, 1::2] = lo, hi
    v = P.int_matmul(a, bt.T) - bt.astype(np.int64).sum(axis=1)[None, :] * zpa
    sigma = float(np.std(v[2:, 3:]))
    kw = dict(zpa=zpa, w_bits=w_bits)
    info = {}
    if epi == "qkv":
        G = N // 3
        k = int(np.rint(np.log2(sigma / 100.0)))
        s_acc = np.array([2.0 ** -12, 2.0 ** -11, 2.0 ** -13], np.float32)
        s_out = (s_acc * np.float32(2.0 ** k)).astype(np.float32)
        zp_out = (3, -9, 20)
        grp = np.repeat(np.arange(3), G)
        bias = (rng.integers(-3000, 3001, size=N).astype(np.float32) * s_acc[grp]).astype(np.float32)
        s = s_acc
        if pc:  # every fourth column keeps the power of two (the tie columns); the others all differ
            s = (s_acc[grp] * np.exp2(rng.uniform(-0.5, 0.5, size=N))).astype(np.float32)
            s[0::4] = s_acc[grp][0::4]
            assert len(set(s[np.arange(N) % 4 != 0].tolist())) == N - N // 4
            other = np.arange(N) % 4 != 0
            bias[other] = (rng.standard_normal(N) * 0.5).astype(np.float32)[other]
        kw.update(bias_h=bias, s_out=tuple(float(x) for x in s_out), zp_out=zp_out)
        kw["tokens"] = tokens
        want = R.fused_qkv(a, bt, bias, zpa, s, kw["s_out"], zp_out, 8, w_bits, tokens, G // 64, 64)
        u, tie = R.fused_qkv_values(a, bt, bias, zpa, s, kw["s_out"], zp_out, 8, w_bits)
        info = dict(low=float(np.mean(u < -128)), high=float(np.mean(u > 127)), ties=int(np.count_nonzero(tie == 0.0)),
                    ties_kept=int(np.count_nonzero((tie == 0.0) & (u >= -128) & (u <= 127))))
    elif epi == "resid":
        s = np.array([np.float32(2.0 / sigma)])
        if pc:
            s = (s[0] * np.exp2(rng.uniform(-2, 2, size=N))).astype(np.float32)
            assert len(set(s.tolist())) == N
        bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
        resid = rng.standard_normal((M, N)).astype(np.float32)
        kw.update(bias_h=bias, resid_h=resid)
        want = [R.fused_resid(a, bt, bias, resid, zpa, s if pc else s[0], w_bits)]
    else:
        s_out, zp_out, sigma_h = GELU_OUT[gelu]
        s = np.array([np.float32(sigma_h / sigma)])
        if pc:
            s = (s[0] * np.exp2(rng.uniform(-0.5, 0.5, size=N))).astype(np.float32)
            assert len(set(s.tolist())) == N
        bias = (rng.standard_normal(N) * 0.3).astype(np.float32)
        kw.update(bias_h=bias, s_out=(s_out,), zp_out=(zp_out,))
        sv = s if pc else s[0]
        want = [R.fused_gelu(a, bt, bias, zpa, sv, s_out, zp_out, 8, w_bits).astype(np.int8)]
        u = R.fused_gelu_values(a, bt, bias, zpa, sv, s_out, zp_out, w_bits)
        info = dict(low=float(np.mean(u < -128)), high=float(np.mean(u > 127)))
    if pc:  # s_acc must not be read beside s_col: another column's scale
        kw.update(s_col=s, s_acc=[float(s[(g * (N // 3) + 1) % N]) for g in range(3)])
    else:
        kw.update(s_acc=[float(x) for x in s] if epi == "qkv" else [float(s[0])])
    info["l1max"] = int(np.abs(bt.astype(np.int64)).sum(axis=1).max())
    return a, bt, kw, want, info


def _check_conditions(epi, a, bt, zpa, want, info, K, w_bits=4):
    """The inputs do what the case is for, on the restatement: the extremes meet, both bounds hold and
    are not slack by more than the zero point's share, both clip bounds are passed by about a tenth,
    ties exist."""
    lo, hi = -(1 << (w_bits - 1)), (1 << (w_bits - 1)) - 1
    assert a.min() == -128 and a.max() == 127 and bt.min() == lo and bt.max() == hi
    assert np.all(a[0] == -128) and np.all(a[1] == 127) and np.all(bt[0] == lo) and np.all(bt[1] == hi)
    b32, b24 = R.pg_bounds(bt, zpa)
    assert info["l1max"] == -lo * K and b32 < 2 ** 31 and b24 < 2 ** 24
    if epi != "resid":
        assert CLIP_LO < info["low"] < CLIP_HI and CLIP_LO < info["high"] < CLIP_HI, info
        assert want[0].min() == -128 and want[0].max() == 127  # the bounds themselves are reached
    if epi == "qkv":
        assert info["ties"] > 0 and info["ties_kept"] > 0, info


PG_CASES = [("qkv", 192, 768, "s8"), ("qkv", 192, 768, "nos8"), ("gelu", 256, 768, "table"), ("gelu", 256, 768, "chain"),
            ("resid", 256, 768, ""), ("resid", 256, 3072, "")]


@pytest.mark.parametrize("zpa", [-128, 0, 127])
@pytest.mark.parametrize("pc", [False, True], ids=["per-tensor", "per-column"])
@pytest.mark.parametrize("M", [PG_BM, PG_BM + 16], ids=["M128", "M144"])
@pytest.mark.parametrize("epi,N,K,variant", PG_CASES, ids=[f"{c[0]}-K{c[2]}{'-' + c[3] if c[3] else ''}" for c in PG_CASES])
def test_fused_gemm_k_pg_nibbles_under_8_bit_activations(epi, N, K, variant, M, pc, zpa, monkeypatch):
    """k_pg's nibble instances with w_bits = 4 and bit_width = 8: QKV on the saturating-store
    instance and, with NQK_PG_NOS8=1, on the clamped one; GELU through a table and, where the
    scale's table does not fit, through the filtered chain; RESID at K = 768 and 3072."""
    if variant == "nos8":
        monkeypatch.setenv("NQK_PG_NOS8", "1")
    else:
        monkeypatch.delenv("NQK_PG_NOS8", raising=False)
    a, bt, kw, want, info = _case(epi, M, N, K, zpa, pc, gelu=variant if epi == "gelu" else "table")
    print(f"{epi} M={M} K={K} zpa={zpa} pc={pc} {variant}: {info}")
    _check_conditions(epi, a, bt, zpa, want, info, K)
    lut = None
    if epi == "gelu":
        lut = _lut(kw["s_out"][0], kw["zp_out"][0])
        print(f"GELU table for s_out={kw['s_out'][0]} zp={kw['zp_out'][0]}: {lut[2]} entries")
        assert (0 < lut[2] <= 512) if variant == "table" else (lut[2] == 0 or lut[2] > 512), lut[2]
        if lut[2] == 0:
            lut = None
    kernel, got = _fused(epi, a, bt, lut=lut, **kw)
    assert kernel == (6 if variant == "table" else 4), kernel
    assert _same(got, want)


def test_k_pg_takes_narrower_weights_and_other_activation_widths():
    """w_bits = 2 and 3 on the same nibble image; bit_width = 6 outputs (no saturating store: the clamp
    follows bit_width, not w_bits)."""
    for w_bits in (3, 2):
        a, bt, kw, want, info = _case("resid", PG_BM + 16, 256, 768, -128, False, w_bits=w_bits)
        _check_conditions("resid", a, bt, -128, want, info, 768, w_bits)
        kernel, got = _fused("resid", a, bt, **kw)
        assert kernel == 4 and _same(got, want)
    a, bt, kw, _, _ = _case("qkv", PG_BM, 192, 768, 127, False)
    want6 = R.fused_qkv(a, bt, kw["bias_h"], 127, np.asarray(kw["s_acc"], np.float32), kw["s_out"], kw["zp_out"], 6, 4, 16, 1, 64)
    kernel, got = _fused("qkv", a, bt, bw=6, **kw)
    assert kernel == 4 and _same(got, want6)
    assert want6[0].min() == -32 and want6[0].max() == 31


# ----------------------------------------------------------------------------- 3. fallbacks
@pytest.mark.parametrize("pc", [False, True], ids=["per-tensor", "per-column"])
@pytest.mark.parametrize("M,K", [(PG_BM + 16, 192), (33, 768)], ids=["K192", "M33"])
@pytest.mark.parametrize("epi,N,variant", [("qkv", 192, ""), ("gelu", 256, "table"), ("gelu", 256, "chain"), ("resid", 256, "")])
def test_fused_gemm_where_k_pg_declines(epi, N, variant, M, K, pc):
    """K = 192 (no nibble instance) and M < PG_BM with the nibble k_pg image offered: k_qgemm_big on
    the nqk_pack_b4 image (1), or with per-column scales k_qgemm_epi on the unpacked weight (0)."""
    a, bt, kw, want, info = _case(epi, M, N, K, -128, pc, gelu=variant or "table")
    _check_conditions(epi, a, bt, -128, want, info, K)
    lut = None
    if epi == "gelu":
        lut = _lut(kw["s_out"][0], kw["zp_out"][0])
        lut = lut if lut[2] > 0 else None
    kernel, got = _fused(epi, a, bt, lut=lut, **kw)
    assert kernel == (0 if pc else 1), kernel
    assert _same(got, want)


def test_fused_gemm_fallbacks_at_an_extreme_zero_point_and_on_k_proj(monkeypatch):
    """An output zero point past 2^20 (k_pg's f32 rounding holds it no longer): k_pg declines and
    k_qgemm_big's f64 quantize takes the nibble image.  (An input zero point cannot make k_pg alone
    decline: nqk_qgemm_fused's own int32 condition, 2^14 K + 128 K |zpa| < 0.98 2^31, is the stricter
    one and refuses a nibble image first.)  NQK_NO_PG=1 at M = 256: the QKV call runs on k_proj (3)."""
    from numpy_quant._lib import NQKError
    for epi, N in (("qkv", 192), ("gelu", 256)):
        a, bt, kw, _, _ = _case(epi, PG_BM, N, 768, 127, False)
        zp = ((1 << 20) + 5, -9, 20) if epi == "qkv" else (-(1 << 20) - 5,)
        kw["zp_out"] = zp
        s = np.asarray(kw["s_acc"], np.float32)
        if epi == "qkv":
            want = R.fused_qkv(a, bt, kw["bias_h"], 127, s, kw["s_out"], zp, 8, 4, 16, 1, 64)
            assert np.all(want[0][:PG_BM] == 127) and len(np.unique(want[1])) > 8
        else:
            want = [R.fused_gelu(a, bt, kw["bias_h"], 127, s[0], kw["s_out"][0], zp[0], 8, 4).astype(np.int8)]
            assert np.all(want[0] == -128)
        kernel, got = _fused(epi, a, bt, **kw)
        assert kernel == 1 and _same(got, want)
    with pytest.raises(NQKError, match="int32"):  # the input zero point's own limit, with its message
        a, bt, kw, _, _ = _case("resid", PG_BM, 256, 768, 25000, False)
        assert R.pg_bounds(bt, 25000)[0] >= 2 ** 31
        _fused("resid", a, bt, **kw)
    a, bt, kw, want, _ = _case("qkv", 256, 768, 768, -128, False, tokens=64)
    kernel, got = _fused("qkv", a, bt, **kw)
    assert kernel == 4 and _same(got, want)
    monkeypatch.setenv("NQK_NO_PG", "1")
    kernel, got = _fused("qkv", a, bt, **kw)
    assert kernel == 3 and _same(got, want)
    monkeypatch.delenv("NQK_NO_PG")
    # a nibble image cannot hold weights said to be wider
    a, bt, kw, _, _ = _case("resid", PG_BM, 256, 768, 0, False)
    with pytest.raises(NQKError, match="w_bits"):
        _fused("resid", a, bt, stated=8, **kw)


# ----------------------------------------------------------------------------- 4. encoder layer
@pytest.fixture(scope="module")
def layer():
    """The spread encoder-layer fixture at batch 2 and the restatement's results per (bit width,
    weight bit width, per_channel), each computed once and left unchanged."""
    proto, graph, x = R.encoder_layer_fixture(MODELS)
    cache = {}

    def ref(bw, wbw, pc=False):
        if (bw, wbw, pc) not in cache:
            qp, qc, axes = R.calibrate(graph, [x], bw, wbw, per_channel=pc)
            vals = R.quantized_forward(graph, qp, qc, [x], bw, weights=axes)
            cache[(bw, wbw, pc)] = (qp, qc, axes, vals, R.outputs_of(graph, vals)[0])
        return cache[(bw, wbw, pc)]

    return proto, graph, x, ref


def _model(proto):
    from numpy_quant.model import Model
    return Model.from_onnx(proto)


def _given(qp):
    from numpy_quant.model import QuantizationParams
    return {k: QuantizationParams(v.scale, v.zero_point) for k, v in qp.items()}


def _check_integers(qmodel, vals, qc):
    """Every quantized value the node loop left equals the restatement's integers, widths and scales."""
    from numpy_quant.tensor import QTensor
    seen = 0
    for v in qmodel.values:
        t = v.data
        want = vals.get(v.name)
        if not isinstance(t, QTensor) or want is None or want[0] != "Q":
            continue
        assert np.array_equal(t.data, want[1]), v.name
        assert t.bit_width == want[2], v.name
        assert np.array_equal(np.asarray(t.scale, np.float32), np.asarray(want[3], np.float32)), v.name
        seen += 1
    assert seen > len(qc)


def _gemm_kernels(monkeypatch):
    """Records (epilogue, M, kernel id) of every nqk_qgemm_fused call the plan makes."""
    from numpy_quant import _lib, plan
    calls = []
    real = plan._gemm

    def spy(epi, a, bt, batch, M, N, K, *rest):
        real(epi, a, bt, batch, M, N, K, *rest)
        calls.append((epi, M, _lib.load().nqk_qgemm_last_kernel()))

    monkeypatch.setattr(plan, "_gemm", spy)
    return calls


@pytest.mark.parametrize("bw,wbw", [(8, 4), (8, 2), (6, 4)])
def test_layer_node_loop_plan_graph_and_blob_equal_the_restatement(layer, bw, wbw, tmp_path, monkeypatch):
    from numpy_quant import blob
    proto, graph, x, ref = layer
    qp, qc, axes, vals, want = ref(bw, wbw)
    model = _model(proto)
    for qmodel in (model.quantize([x], bit_width=bw, weight_bit_width=wbw),
                   model.quantize_with(_given(qp), bit_width=bw, weight_bit_width=wbw)):
        assert qmodel.bit_width == bw and qmodel.weight_bit_width == wbw
        consts = {v.name: v for v in qmodel.values}
        for name in axes:
            assert consts[name].data.bit_width == wbw and np.array_equal(consts[name].data.data, qc[name][1]), name
            assert np.array_equal(np.asarray(qmodel.quant_params[name].scale, np.float32), np.asarray(qp[name].scale, np.float32))
        qmodel.keep_values = True
        eager = qmodel([x])[0]
        assert np.array_equal(eager.view(np.uint32), want.view(np.uint32))
        _check_integers(qmodel, vals, qc)
        qmodel.keep_values = False
    calls = _gemm_kernels(monkeypatch)
    plan = qmodel.compile()
    assert plan.fused == 1
    (step,) = [st for k, st in plan.steps if k == "layer"]
    assert step.wbw == wbw and step.bw == bw
    assert all(step.bp[k][1] == 2 and step.bpg[k].dtype == np.uint8 for k in step.bp)  # nibble images
    out = qmodel([x])[0]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert len(calls) == 8 and all(k in (4, 6) for _, _, k in calls), calls  # two stream halves x four GEMMs on k_pg
    g = qmodel.graph([x])
    try:
        assert g.plan.fused == 1
        assert np.array_equal(g([x])[0].view(np.uint32), out.view(np.uint32))
        x2 = np.ascontiguousarray(x[::-1])
        assert np.array_equal(g([x2])[0].view(np.uint32), want[::-1].view(np.uint32))
    finally:
        g.destroy()
    path = str(tmp_path / "mixed.nqk")
    qmodel.save(path)
    header, _ = blob.read(path)
    assert header["version"] == 3 and header["weight_bit_width"] == wbw and header["bit_width"] == bw
    back = model.load_quantized(path)
    assert back.weight_bit_width == wbw and back.bit_width == bw and not back.per_channel
    back.keep_values = True
    assert np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))
    _check_integers(back, vals, qc)
    back.keep_values = False
    assert np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))


def test_equal_widths_keep_the_blob_bytes_and_the_routes(layer, tmp_path):
    from numpy_quant import blob
    proto, graph, x, ref = layer
    qp = ref(8, 8)[0]
    model = _model(proto)
    files = []
    for wbw in (None, 8):
        q = model.quantize_with(_given(qp), bit_width=8, weight_bit_width=wbw)
        assert q.weight_bit_width == 8
        header, _ = blob.pack(q)
        assert header["version"] == 1 and "weight_bit_width" not in header
        path = str(tmp_path / f"w{wbw}.nqk")
        q.save(path)
        files.append(open(path, "rb").read())
        (step,) = [st for k, st in q.compile().steps if k == "layer"]
        assert step._epi().w_bits == 0 and all(step.bp[k][1] == 1 for k in step.bp)
    assert files[0] == files[1]
    want = ref(8, 8)[4]
    assert np.array_equal(q([x])[0].view(np.uint32), want.view(np.uint32))
    o_qp, o_qc = O.calibrate(graph, [x], 8)
    o_want = O.outputs_of(graph, O.quantized_forward(graph, o_qp, o_qc, [x], 8))[0]
    assert np.array_equal(want.view(np.uint32), o_want.view(np.uint32))


@pytest.mark.parametrize("pc,iconv", [(True, False), (False, True)], ids=["per_channel", "integer_conv"])
def test_layer_beside_per_channel_and_integer_conv(layer, pc, iconv, tmp_path, monkeypatch):
    proto, graph, x, ref = layer
    qp, qc, axes, vals, want = ref(8, 4, pc)
    model = _model(proto)
    qmodel = model.quantize_with(_given(qp), bit_width=8, weight_bit_width=4, per_channel=pc, integer_conv=iconv)
    assert qmodel.per_channel == pc and qmodel.integer_conv == iconv and qmodel.weight_bit_width == 4
    if pc:  # Model.quantize computes the same vectors at the weights' width
        q2 = model.quantize([x], bit_width=8, weight_bit_width=4, per_channel=True)
        for name in axes:
            assert np.array_equal(q2.quant_params[name].scale.view(np.uint32), qp[name].scale.view(np.uint32)), name
    qmodel.keep_values = True
    assert np.array_equal(qmodel([x])[0].view(np.uint32), want.view(np.uint32))
    _check_integers(qmodel, vals, qc)
    qmodel.keep_values = False
    calls = _gemm_kernels(monkeypatch)
    assert qmodel.compile().fused == 1
    assert np.array_equal(qmodel([x])[0].view(np.uint32), want.view(np.uint32))
    assert len(calls) == 8 and all(k in (4, 6) for _, _, k in calls), calls
    path = str(tmp_path / "beside.nqk")
    qmodel.save(path)
    back = model.load_quantized(path)
    assert back.weight_bit_width == 4 and back.per_channel == pc and back.integer_conv == iconv
    assert np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------- 5. classifiers
def _classifier(width=None, batch=2, seed=11):
    from numpy_quant import onnx_proto
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
    if width == 192:
        assert onnx_proto.redimension(proto, 192, 3, 768) > 0
    onnx_proto.rebatch(proto, batch)
    x = np.random.default_rng(seed).standard_normal((batch, 3, 224, 224)).astype(np.float32)
    return proto, x


def test_vit_tiny_classifier_plan_equals_node_loop():
    """ViT-Ti/16 at (8, 4), batch 3: K = 192 has no nibble k_pg instance, so the layers' GEMMs run on the
    big-tile kernel's nibble image; the classifier Gemm (transB) takes the 4-bit weight in the node loop."""
    proto, x = _classifier(192, 3)
    model = _model(proto)
    qmodel = model.quantize([x], bit_width=8, weight_bit_width=4)
    widths = {v.name: v.data.bit_width for v in qmodel.values if hasattr(v.data, "bit_width") and v.data is not None
              and type(v).__name__ == "Constant"}
    assert sorted(set(widths.values())) == [4, 8, 32] and sum(1 for w in widths.values() if w == 4) == 12 * 6 + 1
    qmodel.keep_values = True
    eager = qmodel([x])[0]
    qmodel.keep_values = False
    plan = qmodel.compile()
    assert plan.embeds == 1 and plan.pushdowns == 1 and plan.fused == 12 and plan.cls_tails == 1
    out = qmodel([x])[0]
    assert np.array_equal(out.view(np.uint32), eager.view(np.uint32))
    idx, _ = qmodel.classify([x], k=3)
    assert np.array_equal(idx, np.argsort(-eager, axis=1, kind="stable")[:, :3])


def test_vit_base_classifier_plan_equals_node_loop_on_k_pg(monkeypatch):
    """ViT-Base/16 at (8, 4), batch 2: every projection GEMM of at least PG_BM rows runs on k_pg (4, or 6
    with the GELU table); the rest are the last layer's token-0 tail (one row per image)."""
    proto, x = _classifier(None, 2)
    model = _model(proto)
    qmodel = model.quantize([x], bit_width=8, weight_bit_width=4)
    qmodel.keep_values = True
    eager = qmodel([x])[0]
    qmodel.keep_values = False
    calls = _gemm_kernels(monkeypatch)
    plan = qmodel.compile()
    assert plan.fused == 12 and plan.cls_tails == 1
    out = qmodel([x])[0]
    assert np.array_equal(out.view(np.uint32), eager.view(np.uint32))
    big = [c for c in calls if c[1] >= PG_BM]
    small = [c for c in calls if c[1] < PG_BM]
    assert len(big) == 2 * (11 * 4 + 1) and all(k in (4, 6) for _, _, k in big), big
    assert len(small) == 2 * 3 and all(m == 1 for _, m, _ in small), small  # the tail's out-proj, FFN-up, FFN-down


# ----------------------------------------------------------------------------- 6. error report
def test_compare_reports_a_lower_error_at_w4a8_than_at_w4a4(layer):
    from numpy_quant import compare
    proto, graph, x, ref = layer
    model = _model(proto)
    out_name = graph.outputs[0]
    mse = {}
    for bw, wbw in ((8, 4), (4, 4)):
        q = model.quantize_with(_given(ref(bw, wbw)[0]), bit_width=bw, weight_bit_width=wbw)
        s = model.compare(q, [[x]], k=1).values[out_name]
        mse[(bw, wbw)] = s.mse
        print(f"encoder layer ({bw},{wbw}): output MSE {s.mse:.6g}, SQNR {s.sqnr_db:.3f} dB")
    assert mse[(8, 4)] < mse[(4, 4)]
    reports = compare.sweep(model, [[x]], [[x]], bit_widths=(8,), weight_bit_widths=(8, 4), k=1)
    assert list(reports) == [(8, 8), (8, 4)]
    assert reports[(8, 4)].values[out_name].mse == mse[(8, 4)]
    assert reports[(8, 8)].values[out_name].mse < mse[(8, 4)]
    plain = compare.sweep(model, [[x]], [[x]], bit_widths=(8,), k=1)
    assert list(plain) == [8] and plain[8].values[out_name].mse == reports[(8, 8)].values[out_name].mse
    with pytest.raises(ValueError):
        compare.sweep(model, [[x]], [[x]], bit_widths=(4,), weight_bit_widths=(8,), k=1)
