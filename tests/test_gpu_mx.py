"""OCP Microscaling operands (QModel.mx_format) on the GPU against the NumPy restatement
(tests/_mx_ref.py): nqk_quantize_mx bit for bit, nqk_gemm_mx bit for bit on exactly summable fixtures
and within the float32 summation bound on general data, their refusals, and the node loop of an
encoder layer quantized with the flag.

The general tolerance is measured, not derived.  The derived bound K * 2^-23 * sum_k |a_k b_k| (exact
products, K float32 additions in any order) assumes that the instruction keeps float32 precision while it
aligns its products; with FP8 activations it does not: the largest |out - ref| / sum_k |a_k b_k| over this
file is 4.598e-05 (129, 130, 160, fp8 x fp8; derived 1.907e-05), at most 1.020e-07 with FP4 activations.
REL is twice that maximum at every K, plus one float32 subnormal; an indexing error costs about 1e-1."""
import os

import numpy as np
import pytest

from conftest import ROOT

import _mx_ref as R
import _perchannel_ref as PC

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
BITS = {"mxfp8": 8, "mxfp4": 4}
PAIRS = [("mxfp8", "mxfp8"), ("mxfp8", "mxfp4"), ("mxfp4", "mxfp4")]
REL = 2 * 4.598e-05  # measured (see above)


def _dev(a):
    from numpy_quant.device import DeviceArray
    return DeviceArray.from_host(np.ascontiguousarray(a))


def _within_bound(got, ref, mag, K):
    err = np.abs(got.astype(np.float64) - ref)
    tol = REL * mag + 2.0 ** -149
    print(f"K = {K}: max |out - ref| / sum|a b| = {(err / np.maximum(mag, 1e-300)).max():.3e} (derived {K * 2.0 ** -23:.3e})")
    return got.dtype == np.float32 and got.shape == ref.shape and bool(np.all(err <= tol))


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("rows,cols,ldx", [(1, 32, 32), (5, 96, 96), (130, 160, 160), (11, 160, 163)])
def test_quantize_mx_equals_the_restatement(rows, cols, ldx, fmt):
    """Scaled normal data under the planted blocks; ldx = 163 puts rows at every 4-byte offset within 16, the
    gap columns hold 1e30; ldq = 256 at 160 columns: three padding blocks."""
    from numpy_quant import _lib
    x = R.scaled_normal(rows, cols, 3)
    x[:11] = R.planted_blocks(fmt)[:rows, :cols]
    xs = np.full((rows, ldx), 1e30, np.float32)
    xs[:, :cols] = x
    ldq = (cols + 127) // 128 * 128
    q, s = _dev(np.full((rows, ldq * BITS[fmt] // 8), 0x55, np.uint8)), _dev(np.full((rows, ldq // 32), 3, np.uint8))
    _lib.call("nqk_quantize_mx", _dev(xs).vp, q.vp, s.vp, rows, cols, ldx, ldq, BITS[fmt])
    codes, scales = R.mx_quantize(x, fmt)
    got, got_s = R.unpack(q.to_host(), fmt), s.to_host()
    assert np.array_equal(got_s[:, :cols // 32], scales) and np.all(got_s[:, cols // 32:] == 127)
    assert np.array_equal(got[:, :cols], codes) and not got[:, cols:].any()


def _padded(codes, scales, fmt, ld, fill=0):
    """The stored operand [rows, ld]: zeros and scale 127 from K to the next multiple of 128, `fill` beyond."""
    rows, K = codes.shape
    kp = (K + 127) // 128 * 128
    c = np.full((rows, ld), fill, np.uint8)
    c[:, :kp] = 0
    c[:, :K] = codes
    s = np.full((rows, ld // 32), fill if fill else 127, np.uint8)
    s[:, :kp // 32] = 127
    s[:, :K // 32] = scales
    return R.pack(c, fmt), s


def _gemm_mx(a, sa, fa, bt, sb, fb, lda=None, ldb=None, ldo=None, fill=0):
    from numpy_quant import _lib
    (M, K), N = a.shape, bt.shape[0]
    kp = (K + 127) // 128 * 128
    lda, ldb, ldo = lda or kp, ldb or kp, ldo or N
    ops = [_dev(v) for v in _padded(a, sa, fa, lda, fill) + _padded(bt, sb, fb, ldb, fill)]
    out = _dev(np.full((M, ldo), -7.5, np.float32))
    _lib.call("nqk_gemm_mx", ops[0].vp, ops[1].vp, BITS[fa], ops[2].vp, ops[3].vp, BITS[fb], out.vp, M, N, K, lda, ldb, ldo)
    return out.to_host()


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("M,N,K", [(1, 1, 32), (33, 17, 64), (129, 130, 160), (64, 64, 416)])
def test_gemm_mx_exact_fixtures(M, N, K, fa, fb):
    """Every product is a multiple of 2^-4 and sum |a b| * 2^4 < 2^24: every float32 summation order is exact."""
    a, sa, bt, sb = R.exact_fixture(M, N, K, fa, fb)
    ref, mag = R.mx_matmul_ref(a, sa, fa, bt, sb, fb)
    assert (mag * 16).max() < 2 ** 24 and np.array_equal(ref * 16, np.rint(ref * 16))
    want = ref.astype(np.float32)
    got = _gemm_mx(a, sa, fa, bt, sb, fb)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_gemm_mx_leading_dimensions_and_sentinels(fa, fb):
    """0x55 bytes beyond K's padding to 256 are not read into the result; nothing outside [M][N] is written."""
    M, N, K = 130, 131, 160
    a, sa, bt, sb = R.exact_fixture(M, N, K, fa, fb, seed=1)
    want = R.mx_matmul_ref(a, sa, fa, bt, sb, fb)[0].astype(np.float32)
    got = _gemm_mx(a, sa, fa, bt, sb, fb, lda=384, ldb=512, ldo=136, fill=0x55)
    assert np.array_equal(got[:, :N].view(np.uint32), want.view(np.uint32)) and np.all(got[:, N:] == -7.5)


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("M,N,K", [(129, 130, 160), (127, 160, 768)])
def test_gemm_mx_general_data(M, N, K, fa, fb):
    from numpy_quant import kernels as Kn
    from numpy_quant.tensor import FTensor, QTensor, quantize_tensor_mx
    x, w = R.scaled_normal(M, K, 1), np.ascontiguousarray(R.scaled_normal(N, K, 2).T)
    wq = QTensor(np.zeros((K, N), np.int64), 8, np.float32(1))
    wq._is_weight = True
    assert wq.mx_operand(fb, FTensor(_dev(w))) is wq.mx_operand(fb)  # made once
    prod = quantize_tensor_mx(FTensor(_dev(x)), fa).matmul(wq)
    assert isinstance(prod._unlaunched, Kn.MxProduct) and prod.shape == (M, N)
    for what in ("dev", "data", "T"):
        with pytest.raises(ValueError, match="no integer accumulator"):
            getattr(prod, what)
    with pytest.raises(ValueError, match="left operand only"):
        wq.matmul(quantize_tensor_mx(FTensor(_dev(x)), fa))
    ref, mag = R.mx_matmul_ref(*R.mx_quantize(x, fa), fa, *R.mx_quantize(np.ascontiguousarray(w.T), fb), fb)
    assert _within_bound(prod.dequantize().data, ref, mag, K)


@pytest.mark.parametrize("case", ["q format", "cols%32", "ldq%32", "ldx<cols", "q null", "x misaligned", "a format",
                                  "fp4 x fp8", "K%32", "K=0", "lda%128", "ldb<K", "ldo<N", "a misaligned", "scales null"])
def test_entries_refuse_and_launch_nothing(case):
    from numpy_quant import _lib
    x, q, s = _dev(np.ones((4, 128), np.float32)), _dev(np.full((4, 128), 5, np.uint8)), _dev(np.full((4, 4), 9, np.uint8))
    bt, out = _dev(np.zeros((16, 128), np.uint8)), _dev(np.full((4, 16), 7.0, np.float32))
    qa = dict(x=x.vp, q=q.vp, cols=128, ldx=128, ldq=128, fmt=8)
    ga = dict(a=q.vp, sa=s.vp, fa=8, fb=8, K=128, lda=128, ldb=128, ldo=16)
    upd = {"q format": dict(fmt=6), "cols%32": dict(cols=48), "ldq%32": dict(cols=32, ldq=48), "ldx<cols": dict(ldx=127),
           "q null": dict(q=None), "x misaligned": dict(x=x.ptr + 2), "a format": dict(fa=6), "fp4 x fp8": dict(fa=4),
           "K%32": dict(K=48), "K=0": dict(K=0), "lda%128": dict(lda=160, K=32), "ldb<K": dict(K=256, lda=256),
           "ldo<N": dict(ldo=15), "a misaligned": dict(a=q.ptr + 8), "scales null": dict(sa=None)}[case]
    if set(upd) <= set(qa):
        qa.update(upd)
        with pytest.raises(_lib.NQKError, match="nqk_quantize_mx"):
            _lib.call("nqk_quantize_mx", qa["x"], qa["q"], s.vp, 4, qa["cols"], qa["ldx"], qa["ldq"], qa["fmt"])
    else:
        ga.update(upd)
        with pytest.raises(_lib.NQKError, match="nqk_gemm_mx"):
            _lib.call("nqk_gemm_mx", ga["a"], ga["sa"], ga["fa"], bt.vp, s.vp, ga["fb"], out.vp, 4, 16, ga["K"], ga["lda"],
                      ga["ldb"], ga["ldo"])
    _lib.call("nqk_gemm_mx", q.vp, s.vp, 8, bt.vp, s.vp, 8, out.vp, 0, 16, 128, 128, 128, 16)  # M = 0: nothing
    assert np.all(q.to_host() == 5) and np.all(s.to_host() == 9) and np.all(out.to_host() == 7.0)


@pytest.fixture(scope="module")
def layer_proto():
    return PC.encoder_layer_fixture(MODELS, batch=1)


@pytest.fixture(scope="module")
def layer(layer_proto):
    from numpy_quant.model import Model
    proto, graph, x = layer_proto
    return Model.from_onnx(proto), graph, x


def _check_mx_matmuls(model, qmodel, x, fa, fb):
    """The six MatMuls with a constant weight against the restatement's product of their own input."""
    from numpy_quant.tensor import FTensor
    weights = {v.name: v.data.data for v in model.values if isinstance(v.data, FTensor)}
    qmodel.keep_values = True
    out = qmodel([x])[0]
    assert (qmodel.mx_format, qmodel.mx_weight_format) == (fa, fb) and np.isfinite(out).all()
    assert qmodel.compile().fused == 0
    with pytest.raises(ValueError, match="mx_format"):
        qmodel.save(os.devnull)
    seen = 0
    for node in qmodel.nodes:
        if node.name not in qmodel._mx_nodes or not isinstance(node.inputs[0].data, FTensor):
            continue
        xin, w = node.inputs[0].data.data, weights[node.inputs[1].name]
        K = xin.shape[-1]
        ref, mag = R.mx_matmul_ref(*R.mx_quantize(xin.reshape(-1, K), fa), fa,
                                   *R.mx_quantize(np.ascontiguousarray(w.T), fb), fb)
        got = node.outputs[0].data.dequantize().data
        assert _within_bound(got.reshape(-1, got.shape[-1]), ref, mag, K), node.name
        seen += 1
    assert seen == 6  # Q, K, V, the output projection and the two FFN weights


@pytest.mark.parametrize("fa,fb", [("mxfp8", None), ("mxfp8", "mxfp4")])
def test_layer_matmuls_equal_the_restatement(layer, fa, fb):
    model, graph, x = layer
    _check_mx_matmuls(model, model.quantize([x], mx_format=fa, mx_weight_format=fb), x, fa, fb or fa)


def test_layer_matmuls_at_batch_2(layer_proto):
    import copy
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    proto = copy.deepcopy(layer_proto[0])
    onnx_proto.rebatch(proto, 2)
    x = np.random.default_rng(5).standard_normal((2, 197, 768)).astype(np.float32)
    model = Model.from_onnx(proto)
    _check_mx_matmuls(model, model.quantize([x], mx_format="mxfp8"), x, "mxfp8", "mxfp8")


def test_without_the_format_nothing_changes(layer):
    model, graph, x = layer
    plain, off = model.quantize([x]), model.quantize([x], mx_format=None)
    assert off.mx_format is None and not off._mx_nodes and off.compile().fused == 1
    assert np.array_equal(off([x])[0].view(np.uint32), plain([x])[0].view(np.uint32))


@pytest.mark.parametrize("kw", [dict(per_token=True), dict(group_size=64), dict(weight_clip="mse"), dict(weight_bit_width=4),
                                dict(bit_width=16), dict(mx_format="mxfp4", mx_weight_format="mxfp8")])
def test_quantize_refuses(layer, kw):
    model, graph, x = layer
    with pytest.raises(ValueError, match="mx_format"):
        model.quantize([x], **{"mx_format": "mxfp8", **kw})
