"""Per-token activation scales (QModel.per_token) on the GPU against the NumPy restatement
(tests/_per_token_ref.py), bit for bit: nqk_quantize_rows, nqk_qgemm_rows, their refusals, and the
node loop of an encoder layer quantized with the flag."""
import os

import numpy as np
import pytest

from conftest import ROOT

import _per_token_ref as R
import _perchannel_ref as PC

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


def _dev(a):
    from numpy_quant.device import DeviceArray
    return DeviceArray.from_host(np.ascontiguousarray(a))


def _same(got, want):
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("bit_width", [8, 4, 2])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 768, 4096, 4097])
def test_quantize_rows_equals_the_restatement(cols, rows, bit_width):
    from numpy_quant import _lib
    full = R.row_cases(cols, bit_width)
    ldq = (cols + 15) // 16 * 16
    for x in ([full] if rows == 5 else [full[i:i + 1] for i in range(5)]):
        q, s, z = _dev(np.full((rows, ldq), 0x55, np.int8)), _dev(np.full(rows, -1, np.float32)), _dev(np.full(rows, 99, np.int32))
        xd = _dev(x)
        _lib.call("nqk_quantize_rows", xd.vp, q.vp, s.vp, z.vp, rows, cols, cols, ldq, bit_width)
        wq, ws, wz = R.quantize_rows(x, bit_width)
        got = q.to_host()
        assert np.array_equal(s.to_host().view(np.uint32), ws.view(np.uint32))
        assert np.array_equal(z.to_host(), wz) and wz.min() >= -(1 << (bit_width - 1)) and wz.max() < 1 << (bit_width - 1)
        assert np.array_equal(got[:, :cols], wq) and not got[:, cols:].any()
    if rows == 5 and cols >= 63:
        assert not wq[0].any() and (ws[0], wz[0]) == (1, 0)  # the degenerate row
        assert (ws[4], wz[4]) == (0.5, -1) and ((x[4] / ws[4] % 1) == 0.5).sum() >= cols - 2  # the row of ties


def _quantize_rows(x, cols, ldx, bit_width):
    """(q [rows, cols], pad bytes, s, z) of nqk_quantize_rows on the first `cols` of x [rows, ldx]."""
    from numpy_quant import _lib
    rows, ldq = x.shape[0], (cols + 15) // 16 * 16
    q, s, z = _dev(np.full((rows, ldq), 0x55, np.int8)), _dev(np.full(rows, -1, np.float32)), _dev(np.full(rows, 99, np.int32))
    xd = _dev(x)
    _lib.call("nqk_quantize_rows", xd.vp, q.vp, s.vp, z.vp, rows, cols, ldx, ldq, bit_width)
    got = q.to_host()
    return got[:, :cols], got[:, cols:], s.to_host(), z.to_host()


def _equal_rows(got, want):
    (q, pad, s, z), (wq, ws, wz) = got, want
    return (np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(z, wz) and np.array_equal(q, wq)
            and not pad.any())


@pytest.mark.parametrize("cols", [257, 1021, 4095, 4100, 8195])
def test_quantize_rows_finds_the_extreme_wherever_it_sits(cols):
    """One outlier per row, at the edges of every lane's, wave's and loop trip's share of the row."""
    x, pos = R.extreme_positions(cols, long_path=cols > 4096)
    want = R.quantize_rows(x, 8)
    assert want[1].min() > 3.9  # every row's scale is its outlier's
    assert _equal_rows(_quantize_rows(x, cols, cols, 8), want)


@pytest.mark.parametrize("bit_width", [8, 4])
@pytest.mark.parametrize("cols,ldx", [(64, 67), (4100, 4101)])
def test_quantize_rows_strided_input(cols, ldx, bit_width):
    """ldx odd: rows at every 4-byte offset within 16; the gap columns hold 1e30, which no row's s shows."""
    full = np.concatenate([R.row_cases(cols, bit_width), R.row_cases(cols, bit_width, seed=1)])[:9]
    x = np.full((9, ldx), 1e30, np.float32)
    x[:, :cols] = full
    want = R.quantize_rows(full, bit_width)
    assert want[1].max() < 1e4
    assert _equal_rows(_quantize_rows(x, cols, ldx, bit_width), want)


@pytest.mark.parametrize("bit_width", [8, 4, 2])
def test_quantize_rows_range_extremes(bit_width):
    """An overflowing range (s = inf), FLT_MAX, subnormal scales, a range that underflows to s = 0 at
    8 bits only, the smallest normals, signed zeros (tests/test_per_token_host.py: what they give)."""
    x = R.range_extremes()
    with np.errstate(over="ignore"):
        want = R.quantize_rows(x, bit_width)
    got = _quantize_rows(x, x.shape[1], x.shape[1], bit_width)
    for i in range(x.shape[0]):
        print(f"bits {bit_width} row {i}: s {got[2][i]!r} / {want[1][i]!r}, z {got[3][i]} / {want[2][i]}, "
              f"q {got[0][i, :5]} / {want[0][i, :5]}")
    assert _equal_rows(got, want)


def test_quantize_rows_no_rows():
    from numpy_quant import _lib
    x, q = _dev(np.ones((4, 32), np.float32)), _dev(np.full((4, 32), 5, np.int8))
    s, z = _dev(np.ones(4, np.float32)), _dev(np.ones(4, np.int32))
    _lib.call("nqk_quantize_rows", x.vp, q.vp, s.vp, z.vp, 0, 32, 32, 32, 8)
    for rows, cols in ((-1, 32), (4, 0)):
        with pytest.raises(_lib.NQKError, match="nqk_quantize_rows"):
            _lib.call("nqk_quantize_rows", x.vp, q.vp, s.vp, z.vp, rows, cols, 32, 32, 8)
    assert np.all(q.to_host() == 5) and np.all(s.to_host() == 1) and np.all(z.to_host() == 1)


def _qgemm_rows(a, w, z, s, sw):
    from numpy_quant import kernels as Kn
    bt, col = Kn.weight_bt(_dev(w))
    rq = Kn.RowQuantized(_dev(a), _dev(s), _dev(z.astype(np.int32)), a.shape, 8)
    return Kn.qmatmul_rows(rq, bt, col, _dev(sw)).to_host()


def test_qgemm_rows_integers_beyond_float32():
    """K = 65520, the largest the entry takes, operands near saturation: P - z colsum spans int32 to
    within 1.4 %, |P| alone passes 10^9, and nearly no value has a float32 image
    (tests/test_per_token_host.py asserts it)."""
    a, w, z, s, sw = R.near_limit_operands(40, 48, 65520)
    assert _same(_qgemm_rows(a, w, z, s, sw), R.rows_matmul(a, w, s, z, sw))


def test_qgemm_rows_subnormal_and_overflowing_scales():
    a, w, z, _, _ = R.gemm_operands(33, 48, 96)
    s, sw = R.extreme_scales(33, 48)
    with np.errstate(over="ignore", under="ignore"):
        want = R.rows_matmul(a, w, s, z, sw)
    assert np.isinf(want).any() and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()
    assert _same(_qgemm_rows(a, w, z, s, sw), want)


@pytest.mark.parametrize("K", [16, 80, 768])
@pytest.mark.parametrize("N", [1, 129, 160])
@pytest.mark.parametrize("M", [1, 127, 129])
def test_qgemm_rows_equals_the_restatement(M, N, K):
    from numpy_quant import kernels as Kn
    a, w, z, s, sw = R.gemm_operands(M, N, K)
    bt, col = Kn.weight_bt(_dev(w))
    rq = Kn.RowQuantized(_dev(a), _dev(s), _dev(z.astype(np.int32)), (M, K), 8)
    assert _same(Kn.qmatmul_rows(rq, bt, col, _dev(sw)).to_host(), R.rows_matmul(a, w, s, z, sw))


def test_qgemm_rows_leading_dimensions_and_sentinels():
    from numpy_quant import _lib
    M, N, K, lda, ldb, ldo = 130, 131, 80, 96, 112, 136
    a, w, z, s, sw = R.gemm_operands(M, N, K)
    ap, btp = np.full((M, lda), 77, np.int8), np.full((N, ldb), 77, np.int8)
    ap[:, :K], btp[:, :K] = a, w.T
    out = _dev(np.full((M, ldo), -7.5, np.float32))
    args = [_dev(v) for v in (ap, btp, s, z.astype(np.int32), sw, w.astype(np.int64).sum(axis=0))]
    _lib.call("nqk_qgemm_rows", *(v.vp for v in args), out.vp, M, N, K, lda, ldb, ldo)
    got = out.to_host()
    assert _same(np.ascontiguousarray(got[:, :N]), R.rows_matmul(a, w, s, z, sw)) and np.all(got[:, N:] == -7.5)


@pytest.mark.parametrize("case", ["bits9", "bits1", "ldq<cols", "ldq%16", "ldx<cols", "q null", "x misaligned",
                                  "K>=65536", "K%16", "lda<K", "ldb%16", "ldo<N", "a misaligned", "sw null"])
def test_entries_refuse_and_launch_nothing(case):
    from numpy_quant import _lib
    x, q, out = _dev(np.ones((4, 32), np.float32)), _dev(np.full((4, 32), 5, np.int8)), _dev(np.full((4, 16), 7.0, np.float32))
    s, z, sw, col = _dev(np.ones(4, np.float32)), _dev(np.ones(4, np.int32)), _dev(np.ones(16, np.float32)), _dev(np.ones(16, np.int64))
    bt = _dev(np.ones((16, 32), np.int8))
    qa = dict(x=x.vp, q=q.vp, cols=32, ldx=32, ldq=32, bits=8)
    ga = dict(a=q.vp, sw=sw.vp, K=32, lda=32, ldb=32, ldo=16)
    upd = {"bits9": dict(bits=9), "bits1": dict(bits=1), "ldq<cols": dict(cols=20, ldx=20, ldq=16), "ldq%16": dict(ldq=40),
           "ldx<cols": dict(ldx=31), "q null": dict(q=None), "x misaligned": dict(x=x.ptr + 2), "K>=65536": dict(K=65536, lda=65536, ldb=65536),
           "K%16": dict(K=24), "lda<K": dict(lda=16), "ldb%16": dict(ldb=40), "ldo<N": dict(ldo=15), "a misaligned": dict(a=q.ptr + 8),
           "sw null": dict(sw=None)}[case]
    if set(upd) <= set(qa):
        qa.update(upd)
        with pytest.raises(_lib.NQKError, match="nqk_quantize_rows"):
            _lib.call("nqk_quantize_rows", qa["x"], qa["q"], s.vp, z.vp, 4, qa["cols"], qa["ldx"], qa["ldq"], qa["bits"])
    else:
        ga.update(upd)
        with pytest.raises(_lib.NQKError, match="nqk_qgemm_rows"):
            _lib.call("nqk_qgemm_rows", ga["a"], bt.vp, s.vp, z.vp, ga["sw"], col.vp, out.vp, 4, 16, ga["K"], ga["lda"], ga["ldb"], ga["ldo"])
    assert np.all(q.to_host() == 5) and np.all(out.to_host() == 7.0) and np.all(s.to_host() == 1)


# ----------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def layer_proto():
    return PC.encoder_layer_fixture(MODELS, batch=1)


@pytest.fixture(scope="module")
def layer(layer_proto):
    from numpy_quant.model import Model
    proto, graph, x = layer_proto
    return Model.from_onnx(proto), graph, x


def _check_row_matmuls(qmodel, x, bit_width, per_channel):
    """The six MatMuls with a constant weight against quantize_rows and rows_matmul of their inputs."""
    from numpy_quant.tensor import FTensor
    qmodel.keep_values = True
    out = qmodel([x])[0]
    assert qmodel.per_token and np.isfinite(out).all() and qmodel.compile().fused == 0
    seen = 0
    for node in qmodel.nodes:
        if node.name not in qmodel._row_nodes or not isinstance(node.inputs[0].data, FTensor):
            continue
        w, prod = node.inputs[1].data, node.outputs[0].data
        xin = node.inputs[0].data.data
        sw = np.broadcast_to(np.asarray(qmodel.quant_params[node.inputs[1].name].scale, np.float32), w.data.shape[1:])
        assert sw.ndim == 1 and (np.unique(sw).size > 1) == per_channel
        q, s, z = R.quantize_rows(xin.reshape(-1, xin.shape[-1]), bit_width)
        assert z.min() >= -(1 << (bit_width - 1)) and z.max() < 1 << (bit_width - 1) and q.shape[0] == xin.size // xin.shape[-1]
        want = R.rows_matmul(q, w.data, s, z, np.ascontiguousarray(sw)).reshape(xin.shape[:-1] + (-1,))
        assert _same(prod.dequantize().data, want), node.name
        with pytest.raises(ValueError, match="no integer accumulator"):
            prod.dev
        seen += 1
    assert seen == 6  # Q, K, V, the output projection and the two FFN weights


@pytest.mark.parametrize("per_channel", [False, True])
def test_layer_matmuls_equal_the_restatement(layer, per_channel):
    model, graph, x = layer
    _check_row_matmuls(model.quantize([x], per_token=True, per_channel=per_channel), x, 8, per_channel)


def test_layer_matmuls_at_4_bits(layer):
    """(4, 4): row zero points in -8..7, the quantizer's 4-bit clip feeding the GEMM."""
    model, graph, x = layer
    qmodel = model.quantize([x], per_token=True, bit_width=4, weight_bit_width=4)
    assert qmodel.weight_bit_width == 4
    _check_row_matmuls(qmodel, x, 4, False)


def test_layer_matmuls_at_batch_2(layer_proto):
    """Rows = 2 * 197 = 394: the row index crosses the batch axis (and three row tiles end in a partial one)."""
    import copy
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    proto = copy.deepcopy(layer_proto[0])
    onnx_proto.rebatch(proto, 2)
    x = np.random.default_rng(5).standard_normal((2, 197, 768)).astype(np.float32)
    _check_row_matmuls(Model.from_onnx(proto).quantize([x], per_token=True), x, 8, False)


def test_without_the_flag_nothing_changes(layer):
    model, graph, x = layer
    plain, off = model.quantize([x]), model.quantize([x], per_token=False)
    assert off.per_token is False and not off._row_nodes and off.compile().fused == 1
    assert np.array_equal(off([x])[0].view(np.uint32), plain([x])[0].view(np.uint32))


@pytest.mark.parametrize("kw", [dict(group_size=64), dict(bit_width=16)])
def test_quantize_refuses(layer, kw):
    model, graph, x = layer
    with pytest.raises(ValueError, match="per_token"):
        model.quantize([x], per_token=True, **kw)
