"""Per-column weight scales (QModel.per_channel) on the GPU against the NumPy restatement
(tests/_perchannel_ref.py), bit for bit: the four L1 kernels, the node loop, the plan,
DeviceGraph replay, save / load, the Gemm (transB) case, and the accuracy the feature is for."""
import os

import numpy as np
import pytest

from conftest import ROOT

import _perchannel_ref as R
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


def _dev(a):
    from numpy_quant.device import DeviceArray
    return DeviceArray.from_host(np.ascontiguousarray(a))


def _spread(rng, n, base):
    """n float32 scales spread over 2^-4..2^4 times base, all different: a kernel that reads the
    wrong column's scale cannot pass."""
    s = (np.float32(base) * np.exp2(rng.uniform(-4, 4, size=n))).astype(np.float32)
    assert len(set(s.tolist())) == n
    return s


def _weight(rng, shape):
    k, n = shape
    w = (rng.standard_normal(shape) * np.exp2(rng.uniform(-4, 4, size=n))).astype(np.float32)
    if n > 5:
        w[:, 3] = 0.0                              # an all-zero column
        w[:, 5] = -np.abs(w[:, 5]) - np.float32(0.01)  # a negative-only column
    return w


# ----------------------------------------------------------------------------- L1 kernels
@pytest.mark.parametrize("shape", [(37, 50), (1, 1)])
@pytest.mark.parametrize("bw", [8, 4, 16])
def test_minmax_and_quantize_cols(shape, bw):
    from numpy_quant import kernels as K
    from numpy_quant.model import column_scales
    from numpy_quant.tensor import FTensor
    w = _weight(np.random.default_rng(shape[0] + bw), shape)
    mn, mx = K.minmax_cols(_dev(w))
    assert mn.dtype == np.float32 and np.array_equal(mn, w.min(axis=0)) and np.array_equal(mx, w.max(axis=0))
    s = R.column_scales(w, 1, bw)
    got = column_scales(FTensor(w), 1, bw)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), s.view(np.uint32))
    got0 = column_scales(FTensor(np.ascontiguousarray(w.T)), 0, bw)  # the transB layout
    assert np.array_equal(got0.view(np.uint32), s.view(np.uint32))
    want = R.quantize_cols(w, s, bw)
    q = K.quantize_cols(_dev(w), bw, _dev(s), out_dtype=np.int64).to_host()
    assert np.array_equal(q, want)
    if shape[1] > 5:
        assert np.all(want[:, 3] == -(1 << 63)) and np.all(want[:, 5] == -(1 << (bw - 1)))
    # other scales than the weight's own, and the narrow storage a QTensor uses
    s2 = _spread(np.random.default_rng(bw), shape[1], 0.01)
    want2 = R.quantize_cols(w, s2, bw)
    q2 = K.quantize_cols(_dev(w), bw, _dev(s2))
    assert q2.dtype == K.storage_dtype(bw) and np.array_equal(q2.to_host(), want2.astype(q2.dtype))


def test_minmax_cols_nan_follows_numpy():
    from numpy_quant import kernels as K
    w = np.random.default_rng(0).standard_normal((9, 70)).astype(np.float32)
    w[4, 2] = np.nan
    w[0, 69] = np.nan
    w[1, 7], w[2, 7] = np.inf, -np.inf
    mn, mx = K.minmax_cols(_dev(w))
    assert np.array_equal(mn, w.min(axis=0), equal_nan=True) and np.array_equal(mx, w.max(axis=0), equal_nan=True)
    assert np.isnan(mn[2]) and np.isnan(mx[2]) and np.isnan(mn[69]) and mx[7] == np.inf and mn[7] == -np.inf


@pytest.mark.parametrize("bw", [8, 4, 16])
def test_dequantize_and_requantize_cols(bw):
    """A q_matmul output with both zero points (ROW | COL | KCONST), a batched left operand over
    a 2-D weight (a broadcast bmap) and N = 50, no multiple of 4; then the same with a Gemm bias."""
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    rng = np.random.default_rng(bw)
    lim = 1 << (bw - 1)
    M, Kd, N = 5, 24, 50
    a = rng.integers(-lim, lim, size=(2, M, Kd))
    b = rng.integers(-lim, lim, size=(Kd, N))
    zpa, zpb = np.int64(3), np.int64(-2)
    s_a = np.float32(0.031)
    s_w = _spread(rng, N, 0.004)
    acc, s, zpt = R.q_matmul(a, s_a, zpa, b, s_w, zpb)
    assert s.shape == (N,) and s.dtype == np.float32
    st = K.storage_dtype(bw)
    dacc, zt = K.qmatmul(_dev(a.astype(st)), _dev(b.astype(st)), int(zpa), int(zpb))
    assert zt.flags == _lib.ZP_ROW | _lib.ZP_COL | _lib.ZP_KCONST and zt.b_batch == () and zt.a_batch == (2,)
    assert np.array_equal(dacc.to_host(), acc)
    sdev = _dev(s)
    assert np.array_equal(K.dequantize_cols(dacc, sdev, zt).to_host(), R.dequantize_cols(acc, s, zpt))
    # a plain tensor: scalar zero point, none, 1-D
    assert np.array_equal(K.dequantize_cols(dacc, sdev, 7).to_host(), R.dequantize_cols(acc, s, np.int64(7)))
    assert np.array_equal(K.dequantize_cols(_dev(acc[0, 0]), sdev, None).to_host(), R.dequantize_cols(acc[0, 0], s, None))
    bias = rng.integers(-1000, 1000, size=N)
    for res_zp in (np.int64(-5), None):
        res_scale = np.float32(float(np.abs(R.dequantize_cols(acc, s, zpt)).max()) / lim)
        for bias_h in (None, bias):
            want = R.requantize_cols(acc if bias_h is None else acc + bias_h, s, zpt, res_scale, res_zp, bw)
            got = K.requantize_cols(dacc, sdev, zt, None if bias_h is None else _dev(bias_h), res_scale, res_zp, bw)
            assert np.array_equal(got.to_host(), want), (bw, res_zp, bias_h is None)
            assert len(np.unique(want)) > 4  # the values spread over the range: not all clipped to one end


def test_cols_wrappers_refuse_a_wrong_vector():
    from numpy_quant import kernels as K
    x = _dev(np.zeros((3, 6), np.float32))
    with pytest.raises(ValueError):
        K.quantize_cols(x, 8, _dev(np.ones(5, np.float32)))
    with pytest.raises(ValueError):
        K.dequantize_cols(_dev(np.zeros((3, 6), np.int32)), _dev(np.ones(6, np.float64)), None)
    with pytest.raises(ValueError):
        K.requantize_cols(_dev(np.zeros((3, 6), np.int32)), _dev(np.ones(3, np.float32)), None, None, 1.0, None, 8)


# ----------------------------------------------------------------------------- nqk_qgemm_fused with s_col
SQRT2_F32 = float(np.float32(1.4142135381698608))


def _fused(epi_name, a_h, bt_h, *, zpa, bias_h, s_acc, s_col=None, s_out=(1.0, 1.0, 1.0), zp_out=(0, 0, 0), bw=8,
           resid_h=None, tokens=197, hdim=64, use_col=False, packed=False, pg=None, ln=False, lut=None):
    """One nqk_qgemm_fused call (batch 1) on host operands; returns (kernel id, outputs)."""
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
    e.zp_flags, e.bit_width, e.zpa = _lib.ZP_COL, bw, zpa
    col_h = bt_h.astype(np.int64).sum(axis=1)
    if use_col:
        e.col, e.col_absmax = up(col_h).ptr, int(np.abs(col_h).max())
        e.colterm = up((col_h * zpa).astype(np.int32)).ptr
    e.bias = up(bias_h).ptr
    if s_col is not None:
        e.s_col = up(np.asarray(s_col, np.float32)).ptr
    b_op = bt
    if packed:  # the big-tile kernels' image (the nibble one beside a nibble k_pg image)
        b_op, e.b_packed = _pack_b(bt, 4 if pg == "pg4" else 8)
        keep.append(b_op)
    if pg:  # "pg": nqk_pack_pg, "pg4": nqk_pack_pg4 (b_packed = 2 names it)
        keep.append(_pack_pg(bt, 4 if pg == "pg4" else 8, 1 if epi == EPI_RESID else 0, nibbles=pg == "pg4"))
        assert keep[-1] is not None
        e.bt_pg = keep[-1].ptr
        if pg == "pg4":
            e.b_packed = 2
    if epi == EPI_QKV:
        H = N // 3 // hdim
        e.group_cols, e.tokens, e.heads, e.hdim = N // 3, tokens, H, hdim
        bufs = [DeviceArray((-(-M // tokens) * H * tokens, hdim), np.int8) for _ in range(3)]
        for g in range(3):
            e.s_acc[g], e.s_out[g], e.zp_out[g], e.out[g] = float(s_acc[g]), float(s_out[g]), int(zp_out[g]), bufs[g].ptr
    elif epi == EPI_RESID:
        e.group_cols = 1 << 30
        bufs = [DeviceArray((M, N), np.float32)]
        e.s_acc[0], e.out[0], e.resid = float(s_acc[0]), bufs[0].ptr, up(resid_h).ptr
        if ln:
            bufs.append(DeviceArray((M, N), np.int8))
            e.ln_gamma, e.ln_beta, e.ln_out = up(np.ones(N, np.float32)).ptr, up(np.zeros(N, np.float32)).ptr, bufs[1].ptr
            e.ln_eps, e.ln_scale, e.ln_zp = 1e-5, 0.02, 0
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


def _fused_case(epi, M, N, K, seed=0):
    rng = np.random.default_rng(1000 * M + 10 * N + K + seed)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    bt = rng.integers(-127, 128, size=(N, K), dtype=np.int8)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    s_col = _spread(rng, N, 2.0 / (127 * 127 * np.sqrt(K)))
    zpa = -7
    hdim = 64 if N % 192 == 0 else N // 3
    tokens = 3 if M < 10 else 11  # the last image is partial
    kw = dict(zpa=zpa, bias_h=bias, tokens=tokens, hdim=hdim)
    if epi == "qkv":
        kw.update(s_out=(0.02, 0.05, 0.11), zp_out=(3, -9, 20))
        want = R.fused_qkv(a, bt, bias, zpa, s_col, kw["s_out"], kw["zp_out"], 8, tokens, N // 3 // hdim, hdim)
    elif epi == "resid":
        kw.update(resid_h=rng.standard_normal((M, N)).astype(np.float32))
        want = [R.fused_resid(a, bt, bias, kw["resid_h"], zpa, s_col)]
    else:
        kw.update(s_out=(0.03,), zp_out=(-100,))
        want = [R.fused_gelu(a, bt, bias, zpa, s_col, 0.03, -100, 8).astype(np.int8)]
    return a, bt, s_col, kw, want


def _same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))


@pytest.mark.parametrize("K", [16, 80])
@pytest.mark.parametrize("N", [12, 192])
@pytest.mark.parametrize("M", [5, 33])
@pytest.mark.parametrize("epi", ["qkv", "resid", "gelu"])
def test_fused_gemm_small_tiles_with_s_col(epi, M, N, K):
    a, bt, s_col, kw, want = _fused_case(epi, M, N, K)
    wrong = [float(s_col[(g * (N // 3) + 1) % N]) for g in range(3)]  # s_acc must not be read beside s_col
    kernel, got = _fused(epi, a, bt, s_acc=wrong, s_col=s_col, **kw)
    assert kernel == 0
    assert _same(got, want)
    if epi != "resid":
        assert len(np.unique(want[0])) > 8  # the outputs use their range: not clipped to one end
    # s_col = NULL: all columns equal gives the bytes s_acc gives
    s = float(s_col[0])
    flat = np.full(N, s, np.float32)
    k0, by_vec = _fused(epi, a, bt, s_acc=(s, s, s), s_col=flat, **kw)
    k1, by_acc = _fused(epi, a, bt, s_acc=(s, s, s), s_col=None, **kw)
    assert k0 == 0 and k1 == 0 and _same(by_vec, by_acc)


PG_BM = 128  # nqk_pgemm_kernel.h: k_pg's tile rows


def _pg_case(epi, M, N, nibble, seed=0):
    """Operands of one call k_pg takes: K = 192 with int8 weights; K = 768 with int4-range weights,
    the nibble image and 4-bit outputs (k_pg has no nibble instance at K = 192, with or without
    per-column scales).  QKV: one column per group has a few +-1 weights, zero bias and power-of-two
    scales (c1 = 1/2 exactly), so every odd accumulator of it is a rounding tie: pg_exact_fix's."""
    K, tokens = 768 if nibble else 192, 16
    rng = np.random.default_rng(7000 + 10 * M + N + seed + (1 if nibble else 0))
    wmax, bw = (8, 4) if nibble else (127, 8)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    bt = rng.integers(-8 if nibble else -127, 8 if nibble else 128, size=(N, K)).astype(np.int8)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    s_col = _spread(rng, N, 2.0 / (127 * wmax * np.sqrt(K)))
    zpa = -7
    kw = dict(zpa=zpa, bias_h=bias, tokens=tokens, hdim=64, bw=bw, use_col=True)
    if epi == "qkv":
        s_out, zp_out = ((0.25, 0.5, 1.0), (1, -2, 3)) if nibble else ((2.0 ** -5, 2.0 ** -4, 2.0 ** -3), (3, -9, 20))
        for g, n in enumerate((5, 70, 140)):
            bt[n] = 0
            bt[n, :8] = rng.choice(np.array([-1, 1], np.int8), size=8)
            bias[n] = 0.0
            s_col[n] = np.float32(s_out[g] / 2)
        kw.update(s_out=s_out, zp_out=zp_out)
        want = R.fused_qkv(a, bt, bias, zpa, s_col, s_out, zp_out, bw, tokens, 1, 64)
    elif epi == "resid":
        kw.update(resid_h=rng.standard_normal((M, N)).astype(np.float32))
        want = [R.fused_resid(a, bt, bias, kw["resid_h"], zpa, s_col)]
    else:
        s_out, zp_out = (0.5, -6) if nibble else (0.03, -100)
        kw.update(s_out=(s_out,), zp_out=(zp_out,))
        want = [R.fused_gelu(a, bt, bias, zpa, s_col, s_out, zp_out, bw).astype(np.int8)]
    return a, bt, s_col, kw, want


@pytest.mark.parametrize("nibble", [False, True], ids=["int8", "nibbles"])
@pytest.mark.parametrize("M", [PG_BM, PG_BM + 16], ids=["M128", "M144"])
@pytest.mark.parametrize("epi,N,table", [("qkv", 192, False), ("resid", 256, False), ("gelu", 256, False),
                                         ("gelu", 256, True)])
def test_fused_gemm_k_pg_with_s_col(epi, N, table, M, nibble):
    """k_pg's per-column variant at its smallest shapes (K = 192, nibbles K = 768; M = PG_BM, and one token block
    more: a partial last row tile), int8 and nibble-packed weights, GELU with and without a table.
    s_acc holds another column's scale: no path may read it."""
    from _fused_gpu import build_gelu_lut
    a, bt, s_col, kw, want = _pg_case(epi, M, N, nibble)
    wrong = [float(s_col[(g * (N // 3) + 1) % N]) for g in range(3)]
    lut = None
    if table:
        lut = build_gelu_lut(kw["s_out"][0], kw["zp_out"][0], kw["bw"])
        assert lut[2] > 0
    kernel, got = _fused(epi, a, bt, s_acc=wrong, s_col=s_col, pg="pg4" if nibble else "pg", lut=lut, **kw)
    assert kernel == (6 if table else 4)  # k_pg (6: with the GELU table)
    assert _same(got, want)
    if epi != "resid":
        assert len(np.unique(want[0])) > 8
    if epi == "qkv":
        fixes = R.qkv_exact_fix_count(a, bt, kw["bias_h"], kw["zpa"], s_col, kw["s_out"])
        print(f"QKV M={M} {'nibbles' if nibble else 'int8'}: {fixes} of {M * N} elements take pg_exact_fix")
        assert 0 < fixes < M * N // 10
    # s_col = NULL: all columns equal gives the bytes s_acc gives, on k_pg too
    s = float(s_col[0])
    flat = np.full(N, s, np.float32)
    k0, by_vec = _fused(epi, a, bt, s_acc=(s, s, s), s_col=flat, pg="pg4" if nibble else "pg", lut=lut, **kw)
    k1, by_acc = _fused(epi, a, bt, s_acc=(s, s, s), s_col=None, pg="pg4" if nibble else "pg", lut=lut, packed=True, **kw)
    assert k0 == kernel and k1 == kernel and _same(by_vec, by_acc)


def test_fused_gemm_s_col_where_k_pg_declines_and_refusals():
    """M below PG_BM with the k_pg image offered: the small-tile kernel takes the unpacked bt, also
    beside a nibble image.  ln_out, or an nqk_pack_b image as bt, beside s_col is an error."""
    from numpy_quant._lib import NQKError
    for nibble in (False, True):
        a, bt, s_col, kw, want = _pg_case("resid", 77, 256, nibble)
        s = float(s_col[1])
        kernel, got = _fused("resid", a, bt, s_acc=(s,), s_col=s_col, pg="pg4" if nibble else "pg", **kw)
        assert kernel == 0 and _same(got, want)
    a, bt, s_col, kw, _ = _pg_case("resid", 139, 192, False)
    with pytest.raises(NQKError, match="LayerNorm"):
        _fused("resid", a, bt, s_acc=(s,), s_col=s_col, ln=True, **kw)
    with pytest.raises(NQKError, match="unpacked"):
        _fused("resid", a, bt, s_acc=(s,), s_col=s_col, packed=True, **kw)


# ----------------------------------------------------------------------------- QTensor
def test_qtensor_carries_or_refuses_the_vector():
    from numpy_quant.tensor import FTensor, ITensor, QTensor, quantize_tensor
    rng = np.random.default_rng(3)
    w = _weight(rng, (8, 6))  # stored [N = 8][K = 6], as a Gemm with transB keeps it
    s = R.column_scales(w, 0, 8)
    qt = quantize_tensor(FTensor(w), 8, s, None, scale_axis=0)
    assert qt.per_column and qt.scale_axis == 0
    assert np.array_equal(qt.data, R.quantize_cols(w, s, 8, axis=0))
    t = qt.T
    assert t.scale_axis == -1 and t.shape == (6, 8) and np.array_equal(t.data, qt.data.T)
    assert np.array_equal(t.dequantize().data, R.dequantize_cols(qt.data.T, s, None))
    assert np.array_equal(qt.dequantize().data, R.dequantize_cols(qt.data.T, s, None).T)
    assert t.transpose([1, 0]).scale_axis == 0
    assert t.reshape(ITensor(np.array([2, 3, 8]))).shape == (2, 3, 8)
    with pytest.raises(ValueError):
        t.reshape(ITensor(np.array([8, 6])))
    with pytest.raises(ValueError):
        t.reshape(ITensor(np.array([2, 3, 8]))).transpose([0, 2, 1])
    x = quantize_tensor(FTensor(rng.standard_normal((4, 6)).astype(np.float32)), 8, np.float32(0.02), np.int64(1))
    out = x.matmul(t)
    assert out.per_column and np.array_equal(out.scale, np.float32(0.02) * s)
    with pytest.raises(ValueError):
        x.matmul(qt)       # the vector on the K axis
    with pytest.raises(ValueError):
        t.matmul(x.T)      # a per-column left operand
    with pytest.raises(ValueError):
        QTensor(np.zeros((6, 8), np.int64), 8, s, np.int64(2))  # no scalar zero point beside a vector
    with pytest.raises(ValueError):
        QTensor(np.zeros((6, 7), np.int64), 8, s)


# ----------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def layer():
    """The encoder-layer fixture, its float outputs and the restatement's results per
    (bit width, per_channel), each computed once and left unchanged."""
    proto, graph, x = R.encoder_layer_fixture(MODELS)
    cache = {}

    def ref(bw, pc=True):
        if (bw, pc) not in cache:
            qp, qc, axes = R.calibrate(graph, [x], bw, per_channel=pc)
            vals = R.quantized_forward(graph, qp, qc, [x], bw)
            cache[(bw, pc)] = (qp, qc, axes, vals, R.outputs_of(graph, vals)[0])
        return cache[(bw, pc)]

    return proto, graph, x, ref


def _model(proto):
    from numpy_quant.model import Model
    return Model.from_onnx(proto)


def _given(qp):
    from numpy_quant.model import QuantizationParams
    return {k: QuantizationParams(v.scale, v.zero_point) for k, v in qp.items()}


def _check_integers(qmodel, vals, qc):
    """Every quantized value the node loop left equals the restatement's integers and scales."""
    from numpy_quant.tensor import QTensor
    seen = 0
    for v in qmodel.values:
        t = v.data
        want = vals.get(v.name)
        if not isinstance(t, QTensor) or want is None or want[0] != "Q":
            continue
        assert np.array_equal(t.data, want[1]), v.name
        assert np.array_equal(np.asarray(t.scale, np.float32), np.asarray(want[3], np.float32)), v.name
        assert t.per_column == (np.ndim(want[3]) == 1), v.name
        seen += 1
    assert seen > len(qc)  # the constants and the MatMul outputs


@pytest.mark.parametrize("bw", [8, 4])
def test_layer_node_loop_and_plan_equal_the_restatement(layer, bw):
    proto, graph, x, ref = layer
    qp, qc, axes, vals, want = ref(bw)
    assert len(axes) == 6
    model = _model(proto)
    qmodel = model.quantize_with(_given(qp), bit_width=bw, per_channel=True)
    assert qmodel.per_channel
    qmodel.keep_values = True
    eager = qmodel([x])[0]
    assert np.array_equal(eager.view(np.uint32), want.view(np.uint32))
    _check_integers(qmodel, vals, qc)
    qmodel.keep_values = False
    plan = qmodel.compile()
    assert plan.fused == 1  # the layer's four GEMMs run nqk_qgemm_fused with s_col
    (layer_step,) = [st for k, st in plan.steps if k == "layer"]
    assert layer_step.pc and not layer_step.ln_fuse and set(layer_step.scol) == {"qkv", "o", "1", "2"}
    assert np.array_equal(layer_step.scol["qkv"].to_host(),
                          np.concatenate([np.float32(qp[layer_step.m.ln1_out.name].scale) * qp[layer_step.m.roles[r]["w"].name].scale
                                          for r in "qkv"]))
    assert np.array_equal(qmodel([x])[0].view(np.uint32), want.view(np.uint32))
    # the default stays what it was: the same parameters without the vectors are refused, and a
    # per-tensor model of the same graph gives the per-tensor restatement
    with pytest.raises(ValueError):
        model.quantize_with(_given(qp), bit_width=bw)
    qp_t, _, _, _, want_t = ref(bw, False)
    q_t = model.quantize_with(_given(qp_t), bit_width=bw)
    assert not q_t.per_channel
    assert np.array_equal(q_t([x])[0].view(np.uint32), want_t.view(np.uint32))


@pytest.mark.parametrize("bw", [8, 4])
def test_quantize_computes_the_column_scales_on_the_device(layer, bw):
    """Model.quantize(per_channel=True): the weights' vectors and integers depend on the weights
    alone and equal the restatement's; the plan equals the node loop."""
    proto, graph, x, ref = layer
    qp, qc, axes, _, _ = ref(bw)
    qmodel = _model(proto).quantize([x], bit_width=bw, per_channel=True)
    consts = {v.name: v for v in qmodel.values}
    for name in axes:
        s = qmodel.quant_params[name].scale
        assert s.dtype == np.float32 and np.array_equal(s.view(np.uint32), qp[name].scale.view(np.uint32)), name
        assert qmodel.quant_params[name].zero_point is None
        assert np.array_equal(consts[name].data.data, qc[name][1]), name
    for name, p in qmodel.quant_params.items():
        assert name in axes or np.ndim(p.scale) == 0, name  # everything else keeps one scale
    qmodel.keep_values = True
    eager = qmodel([x])[0]
    qmodel.keep_values = False
    assert np.array_equal(qmodel([x])[0].view(np.uint32), eager.view(np.uint32))
    assert qmodel._plan.fused == 1


def test_layer_graph_replay_save_load_and_integer_conv(layer, tmp_path):
    proto, graph, x, ref = layer
    bw = 8
    qp, qc, axes, vals, want = ref(bw)
    model = _model(proto)
    qmodel = model.quantize_with(_given(qp), bit_width=bw, per_channel=True, integer_conv=True)
    assert qmodel.per_channel and qmodel.integer_conv
    g = qmodel.graph([x])
    try:
        assert g.plan.fused == 1
        assert np.array_equal(g([x])[0].view(np.uint32), want.view(np.uint32))
        x2 = np.ascontiguousarray(x[::-1])
        assert np.array_equal(g([x2])[0].view(np.uint32), want[::-1].view(np.uint32))  # rows are independent
    finally:
        g.destroy()
    path = str(tmp_path / "pc.nqk")
    qmodel.save(path)
    back = model.load_quantized(path)
    assert back.per_channel and back.integer_conv and back.bit_width == bw
    for name in axes:
        assert np.array_equal(back.quant_params[name].scale.view(np.uint32), qp[name].scale.view(np.uint32))
    back.keep_values = True
    assert np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))
    _check_integers(back, vals, qc)
    back.keep_values = False
    assert np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))
    # a model saved without the flag keeps the version-1 header
    from numpy_quant import blob
    plain = model.quantize_with(_given(ref(bw, False)[0]), bit_width=bw)
    header, _ = blob.pack(plain)
    assert header["version"] == 1 and "per_channel" not in header
    assert blob.pack(qmodel)[0]["version"] == 2


@pytest.mark.parametrize("bw", [8, 4])
def test_gemm_transb_model_equals_the_restatement(bw, tmp_path):
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    path = os.path.join(MODELS, "mlp.onnx")
    x = np.random.default_rng(0).uniform(-1.2, 1.2, size=(64, 2)).astype(np.float32)
    graph = O.Graph(onnx_proto.load(path))
    qp, qc, axes = R.calibrate(graph, [x], bw)
    assert axes and set(axes.values()) == {0}
    vals = R.quantized_forward(graph, qp, qc, [x], bw)
    want = R.outputs_of(graph, vals)[0]
    model = Model.from_onnx(path)
    for qmodel in (model.quantize([x], bit_width=bw, per_channel=True),
                   model.quantize_with(_given(qp), bit_width=bw, per_channel=True)):
        for name, axis in axes.items():
            t = {v.name: v for v in qmodel.values}[name].data
            assert t.scale_axis == 0 and np.array_equal(t.scale.view(np.uint32), qp[name].scale.view(np.uint32))
        qmodel.keep_values = True
        assert np.array_equal(qmodel([x])[0].view(np.uint32), want.view(np.uint32))
        _check_integers(qmodel, vals, qc)
        qmodel.keep_values = False
        assert np.array_equal(qmodel([x])[0].view(np.uint32), want.view(np.uint32))
    p = str(tmp_path / "mlp.nqk")
    qmodel.save(p)
    back = model.load_quantized(p)
    assert back.per_channel and np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))
    idx, prob = back.classify([x], k=1)
    assert idx.shape == (64, 1)


def test_quantize_stream_refuses_clipped_weights(layer):
    proto, _, x, _ = layer
    model = _model(proto)
    with pytest.raises(ValueError, match="per_channel"):
        model.quantize_stream([[x]], bit_width=8, percentile=99.9, clip_weights=True, per_channel=True)
    q = model.quantize_stream([[x]], bit_width=8, per_channel=True)
    assert q.per_channel


def test_per_channel_lowers_the_4_bit_output_error(layer):
    """The point of the feature: on the same batches Model.compare reports a lower output MSE
    for the per-channel QModel than for the per-tensor one (the strict inequality only)."""
    proto, graph, x, ref = layer
    model = _model(proto)
    out_name = graph.outputs[0]
    mse = {}
    for pc in (False, True):
        q = model.quantize_with(_given(ref(4, pc)[0]), bit_width=4, per_channel=pc)
        rep = model.compare(q, [[x]], k=1)
        s = rep.values[out_name]
        mse[pc] = s.mse
        print(f"4-bit encoder layer, per_channel={pc}: output MSE {s.mse:.6g}, SQNR {s.sqnr_db:.3f} dB")
        for name in ref(4, True)[2]:
            assert name in rep.values and rep.values[name].count == graph.constants[name].size
    assert mse[True] < mse[False]


def test_vit_tiny_classifier_plan_graph_and_classify(tmp_path):
    """The whole classifier (ViT-Ti/16, batch 2, 8 bits) with per_channel: the fused embedding, the
    LayerNorm/Gather pushdown and the transB classifier Gemm beside the per-column MatMuls.  The
    node loop equals the restatement in every output bit, the plan, a graph replay, classify and
    a reloaded blob equal the node loop."""
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
    assert onnx_proto.redimension(proto, 192, 3, 768) > 0
    onnx_proto.rebatch(proto, 2)
    graph = O.Graph(proto)
    x = np.random.default_rng(11).standard_normal((2, 3, 224, 224)).astype(np.float32)
    qp, qc, axes = R.calibrate(graph, [x], 8)
    assert len(axes) == 12 * 6 + 1 and sorted(set(axes.values())) == [0, 1]  # the classifier Gemm has transB
    want = R.outputs_of(graph, R.quantized_forward(graph, qp, qc, [x], 8))[0]
    model = Model.from_onnx(proto)
    qmodel = model.quantize_with(_given(qp), bit_width=8, per_channel=True)
    qmodel.keep_values = True
    eager = qmodel([x])[0]
    assert np.array_equal(eager.view(np.uint32), want.view(np.uint32))
    qmodel.keep_values = False
    plan = qmodel.compile()
    assert plan.embeds == 1 and plan.pushdowns == 1 and plan.fused == 12 and plan.cls_tails == 1
    assert np.array_equal(qmodel([x])[0].view(np.uint32), want.view(np.uint32))
    idx, prob = qmodel.classify([x], k=3)
    assert np.array_equal(idx, np.argsort(-want, axis=1, kind="stable")[:, :3])
    g = qmodel.graph([x])
    try:
        assert np.array_equal(g([x])[0].view(np.uint32), want.view(np.uint32))
    finally:
        g.destroy()
    path = str(tmp_path / "tiny_pc.nqk")
    qmodel.save(path)
    back = model.load_quantized(path)
    assert back.per_channel and np.array_equal(back([x])[0].view(np.uint32), want.view(np.uint32))
