"""Group-wise weight scales (QModel.group_size) on the GPU against the NumPy restatement
(tests/_group_ref.py), bit for bit: nqk_qgemm_group and nqk_group_colsum, their refusals, the node
loop of a grouped encoder layer, and the argument errors."""
import os

import numpy as np
import pytest

from conftest import ROOT

import _group_ref as R
import _perchannel_ref as PC
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


def _dev(a):
    from numpy_quant.device import DeviceArray
    return DeviceArray.from_host(np.ascontiguousarray(a))


def _run(a, b, sg, zpa, g):
    from numpy_quant import kernels as K
    bt, _ = K.weight_bt(_dev(b))
    gsum = K.group_colsum(bt, g)
    assert np.array_equal(gsum.to_host(), b.astype(np.int64).reshape(-1, g, b.shape[1]).sum(axis=1))
    return K.qmatmul_group(_dev(a), bt, gsum, _dev(sg), zpa, g).to_host()


def _same(got, want):
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("zpa", R.ZPS)
@pytest.mark.parametrize("M,N,K,g", R.SHAPES)
def test_kernel_equals_the_restatement(M, N, K, g, zpa):
    a, b, sg = R.operands(M, N, K, g)
    assert _same(_run(a, b, sg, zpa, g), R.group_matmul(a, b, sg, zpa, g))


def test_saturating_operands():
    """All a = -128 with zpa = 127, all b = -128, g = 256: |P_j| = 255 * 128 * 256, the largest a
    group of 256 reaches (just below 2^24)."""
    a, b = np.full((40, 512), -128, np.int8), np.full((512, 48), -128, np.int8)
    sg = R.operands(40, 48, 512, 256)[2]
    want = R.group_matmul(a, b, sg, 127, 256)
    assert R.group_products(a, b, 127, 256).max() == 255 * 128 * 256
    assert _same(_run(a, b, sg, 127, 256), want)


@pytest.mark.parametrize("M,N,g", [(40, 48, 16384), (130, 131, 4096)])
def test_partial_sums_beyond_float32(M, N, g):
    """|P_j| just below 255 * 128 * g, 2^29 at the largest g the entry takes: nearly no P_j has a
    float32 image (tests/test_group_host.py asserts it), so a conversion or a multiply through
    float32 changes about a quarter of the outputs."""
    a, b, sg = R.near_limit_operands(M, N, g)
    assert _same(_run(a, b, sg, 127, g), R.group_matmul(a, b, sg, 127, g))


@pytest.mark.parametrize("zpa", [None, 5])
def test_subnormal_and_overflowing_scales(zpa):
    a, b, _ = R.operands(33, 48, 96, 32)
    sg = R.extreme_scale_rows(48)
    with np.errstate(over="ignore", under="ignore"):
        want = R.group_matmul(a, b, sg, zpa, 32)
    assert np.isinf(want).any() and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()
    assert _same(_run(a, b, sg, zpa, 32), want)


@pytest.mark.parametrize("zpa", R.ZPS)
@pytest.mark.parametrize("M,N,K,g", [(130, 131, 288, 96), (33, 48, 320, 160)])
def test_groups_of_an_odd_number_of_k_steps(M, N, K, g, zpa):
    """g / 32 odd: the group boundaries fall alternately in the middle and at the end of a 64-wide k-tile."""
    a, b, sg = R.operands(M, N, K, g)
    assert _same(_run(a, b, sg, zpa, g), R.group_matmul(a, b, sg, zpa, g))


@pytest.mark.parametrize("zpa", [None, 127])
def test_64_groups_are_added_in_order(zpa):
    """Operands whose float32 result depends on the order of the f64 additions (tests/test_group_host.py)."""
    a, b, sg = R.many_group_operands(70, 136)
    assert _same(_run(a, b, sg, zpa, 32), R.group_matmul(a, b, sg, zpa, 32))


def test_leading_dimensions_and_sentinels():
    from numpy_quant import _lib
    M, N, K, g, lda, ldb, ldo, zpa = 130, 131, 192, 96, 208, 224, 136, 5
    a, b, sg = R.operands(M, N, K, g)
    ap, btp = np.full((M, lda), 77, np.int8), np.full((N, ldb), 77, np.int8)
    ap[:, :K], btp[:, :K] = a, b.T
    G = K // g
    ad, btd, sgd = _dev(ap), _dev(btp), _dev(sg)
    gsum, out = _dev(np.full(G * N + 64, -9, np.int32)), _dev(np.full((M, ldo), -7.5, np.float32))
    _lib.call("nqk_group_colsum", btd.vp, N, K, ldb, g, gsum.vp)
    gs = gsum.to_host()
    assert np.array_equal(gs[:G * N].reshape(G, N), b.astype(np.int64).reshape(G, g, N).sum(axis=1)) and np.all(gs[G * N:] == -9)
    _lib.call("nqk_qgemm_group", ad.vp, btd.vp, sgd.vp, gsum.vp, out.vp, M, N, K, lda, ldb, ldo, g, zpa, 1)
    got = out.to_host()
    assert _same(np.ascontiguousarray(got[:, :N]), R.group_matmul(a, b, sg, zpa, g)) and np.all(got[:, N:] == -7.5)


def test_group_colsum_grid_stride():
    """G N = 1 048 640 sums, above the 4096 x 256 threads the launch is capped at: the last 64 are a
    thread's second trip."""
    from numpy_quant import kernels as K
    N, g = 524320, 32
    bt = np.random.default_rng(3).integers(-128, 128, size=(N, 2 * g), dtype=np.int8)
    assert 2 * N > 4096 * 256
    got = K.group_colsum(_dev(bt), g).to_host()
    assert got.dtype == np.int32 and np.array_equal(got, bt.reshape(N, 2, g).sum(axis=2, dtype=np.int64).T)


def test_batch_axis_folds_into_m():
    a, b, sg = R.operands(3 * 50, 80, 128, 32)
    got = _run(a.reshape(3, 50, 128), b, sg, -3, 32)
    assert got.shape == (3, 50, 80) and _same(got, R.group_matmul(a, b, sg, -3, 32).reshape(3, 50, 80))


@pytest.mark.parametrize("g", [64, 128])
def test_one_group_equals_the_per_column_route(g):
    from numpy_quant import kernels as K
    a, b, sg = R.operands(64, 48, g, g)
    acc, zt = K.qmatmul(_dev(a), _dev(b), 9, None)
    assert acc.dtype == np.int32  # nqk_qgemm_i8
    assert _same(_run(a, b, sg, 9, g), K.dequantize_cols(acc, _dev(sg[0]), zt).to_host())


@pytest.mark.parametrize("case", ["g48", "K%g", "misaligned"])
def test_entries_refuse_and_launch_nothing(case):
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    a, b, sg = R.operands(32, 32, 96, 32)
    bt, _ = K.weight_bt(_dev(b))
    ad, sgd, gsum = _dev(a), _dev(sg), _dev(np.ones((3, 32), np.int32))
    out = _dev(np.full((32, 32), 7.0, np.float32))
    g, ap = {"g48": (48, ad.ptr), "K%g": (64, ad.ptr), "misaligned": (32, ad.ptr + 1)}[case]
    with pytest.raises(_lib.NQKError, match="nqk_qgemm_group"):
        _lib.call("nqk_qgemm_group", ap, bt.vp, sgd.vp, gsum.vp, out.vp, 32, 32, 96, 96, 96, 32, g, 1, 1)
    with pytest.raises(_lib.NQKError, match="nqk_group_colsum"):
        _lib.call("nqk_group_colsum", bt.ptr + 1 if case == "misaligned" else bt.vp, 32, 96, 96, g, gsum.vp)
    assert np.all(out.to_host() == 7.0) and np.all(gsum.to_host() == 1)


@pytest.mark.parametrize("case", ["g16416", "ldo<N", "lda<K", "zpa128", "gsum null", "sg null", "M0"])
def test_more_refusals_and_no_rows(case):
    """Every buffer has the size the refused call names, and M = 0 returns 0; nothing is written."""
    from numpy_quant import _lib
    g = 16416 if case == "g16416" else 32
    M, N, K = 32, 32, 3 * g if g == 32 else g
    ad, bt = _dev(np.ones((M, K), np.int8)), _dev(np.ones((N, K), np.int8))
    sgd, gsum = _dev(np.ones((K // g, N), np.float32)), _dev(np.ones((K // g, N), np.int32))
    out = _dev(np.full((M, N), 7.0, np.float32))
    kw = dict(sg=sgd.vp, gsum=gsum.vp, M=M, lda=K, ldo=N, zpa=5)
    kw.update({"g16416": {}, "ldo<N": dict(ldo=N - 1), "lda<K": dict(lda=K - 16), "zpa128": dict(zpa=128),
               "gsum null": dict(gsum=None), "sg null": dict(sg=None), "M0": dict(M=0)}[case])
    args = (ad.vp, bt.vp, kw["sg"], kw["gsum"], out.vp, kw["M"], N, K, kw["lda"], K, kw["ldo"], g, kw["zpa"], 1)
    if case == "M0":
        _lib.call("nqk_qgemm_group", *args)
    else:
        with pytest.raises(_lib.NQKError, match="nqk_qgemm_group"):
            _lib.call("nqk_qgemm_group", *args)
    if case == "g16416":
        with pytest.raises(_lib.NQKError, match="nqk_group_colsum"):
            _lib.call("nqk_group_colsum", bt.vp, N, K, K, g, gsum.vp)
    assert np.all(out.to_host() == 7.0) and np.all(gsum.to_host() == 1)


# ----------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def layer():
    """The encoder layer with the per-channel tests' seeded stand-in weights, batch 1, quantized at
    (8, 4) with groups of 64, after one forward of the node loop."""
    from numpy_quant.model import Model
    proto, graph, x = PC.encoder_layer_fixture(MODELS, batch=1)
    model = Model.from_onnx(proto)
    qmodel = model.quantize([x], bit_width=8, weight_bit_width=4, group_size=64)
    qmodel.keep_values = True
    return model, graph, x, qmodel, qmodel([x])[0]


def test_layer_matmuls_and_weights_equal_the_restatement(layer):
    from numpy_quant.tensor import FTensor
    model, graph, x, qmodel, out = layer
    assert qmodel.group_size == 64 and qmodel.weight_bit_width == 4
    seen = 0
    for node in qmodel.nodes:
        w = node.inputs[1].data if node.op == "MatMul" else None
        if w is None or getattr(w, "group_size", None) is None:
            continue
        name = node.inputs[1].name
        S = R.group_scales(graph.constants[name], 64, 4)
        assert np.array_equal(qmodel.quant_params[name].scale.view(np.uint32), S.view(np.uint32)), name
        assert np.array_equal(w.data, R.quantize_group(graph.constants[name], S, 64, 4)), name
        assert _same(w.dequantize().data, (w.data * np.repeat(S.astype(np.float64), 64, axis=0)).astype(np.float32))
        xin, p = node.inputs[0].data, qmodel.quant_params[node.inputs[0].name]
        a = O.quantize(xin.data, 8, p.scale, p.zero_point) if isinstance(xin, FTensor) else xin.data
        sg = (np.float32(p.scale) * S).astype(np.float32)
        zpa = None if p.zero_point is None else int(p.zero_point)
        assert _same(node.outputs[0].data.dequantize().data, R.group_matmul(a, w.data, sg, zpa, 64)), node.name
        for what in ("dev", "data", "T"):
            with pytest.raises(ValueError, match="no integer accumulator"):
                getattr(node.outputs[0].data, what)
        seen += 1
    assert seen == 6  # Q, K, V, the output projection and the two FFN weights
    assert qmodel.compile().fused == 0


def test_layer_forward_repeats_and_none_changes_nothing(layer):
    model, graph, x, qmodel, out = layer
    assert np.array_equal(qmodel([x])[0].view(np.uint32), out.view(np.uint32))
    plain = model.quantize([x], bit_width=8, weight_bit_width=4)([x])[0]
    none = model.quantize([x], bit_width=8, weight_bit_width=4, group_size=None)
    assert none.group_size is None and np.array_equal(none([x])[0].view(np.uint32), plain.view(np.uint32))
    assert not np.array_equal(out, plain)
    rep = model.compare(qmodel, [[x]], k=1)
    s = rep.values[graph.outputs[0]]
    print(f"(8, 4) encoder layer, group_size=64: output MSE {s.mse:.6g}, SQNR {s.sqnr_db:.3f} dB")
    assert s.count == out.size and np.isfinite(s.mse)


@pytest.mark.parametrize("kw", [dict(group_size=48), dict(group_size=64, bit_width=16),
                                dict(group_size=64, weight_clip="mse", weight_bit_width=4)])
def test_quantize_refuses(layer, kw):
    model, graph, x, qmodel, out = layer
    with pytest.raises(ValueError, match="group_size"):
        model.quantize([x], **kw)


def test_save_refuses(layer, tmp_path):
    with pytest.raises(ValueError, match="group"):
        layer[3].save(str(tmp_path / "g.nqk"))
