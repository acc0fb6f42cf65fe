"""The weight clipping search on the GPU: nqk_clip_search_cols against the NumPy restatement
(tests/_clip_ref.py) in bits, and Model.quantize(weight_clip="mse") against quantize_with fed the
restatement's scales: weights, scales and output bits, through the node loop and the fused plan."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT

import _clip_ref as R
import _mixed_ref as M
import _perchannel_ref as P

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


def _search(w, s0, ratio, bw, ld=None, offset=0):
    """The kernel on w stored with row stride ld, `offset` floats into a buffer of NaN around it."""
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rows, cols = w.shape
    ld = cols if ld is None else ld
    host = np.full(offset + rows * ld + 5, np.nan, np.float32)
    host[offset:offset + rows * ld].reshape(rows, ld)[:, :cols] = w
    buf = DeviceArray.from_host(host).offset_view(offset, (rows * ld,))
    return [a.to_host() for a in K.clip_search_cols(buf, s0, ratio, bw, want_err=True, rows=rows, cols=cols, ld=ld)]


def _check(got, want):
    """scale, index and err in bits (a NaN err for a NaN err)."""
    (scale, index, err), (rs, ri, re) = got, want
    assert scale.dtype == np.float32 and index.dtype == np.int32 and err.dtype == np.float64 and err.shape == re.shape
    assert np.array_equal(scale.view(np.uint32), rs.view(np.uint32)) and np.array_equal(index, ri)
    nan = np.isnan(re)
    assert np.array_equal(np.isnan(err), nan) and np.array_equal(err[~nan].view(np.uint64), re[~nan].view(np.uint64))
    cols = np.arange(index.shape[0])
    assert not (err[index, cols] > err[0]).any()  # never worse than the scale without the search


# rows below, at and past one round of the 64 partials and a ragged tail; a workgroup owns one column:
# 1, 2 and 70 of them, the last also in padded rows behind an offset pointer; every case takes the
# next candidate count (one, two, past half the waves' 16 each, all) and the next width of 2, 4, 8
SHAPES = [(rows, cols, ld, off) for rows in (1, 63, 64, 65, 200) for cols, ld, off in ((1, 1, 0), (2, 2, 0), (70, 70, 0), (70, 75, 3))]
CASES = [s + ((1, 2, 33, 64)[i % 4], (2, 4, 8)[i % 3]) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("rows,cols,ld,off,G,bw", CASES)
def test_kernel_equals_the_restatement(rows, cols, ld, off, G, bw):
    rng = np.random.default_rng(rows * 100 + cols + off)
    w = (rng.standard_normal((rows, cols)) * np.exp2(rng.uniform(-3, 3, cols))).astype(np.float32)
    w[rng.random((rows, cols)) < 0.02] *= 6  # a few wide entries, which a narrower scale clips
    s0 = P.column_scales(w, 1, bw)
    ratio = R.ratios(G)
    _check(_search(w, s0, ratio, bw, ld, off), R.search_cols(w, s0, ratio, bw))


@pytest.mark.parametrize("bw", [2, 4, 8])
def test_kernel_special_columns(bw):
    """Columns: 0 all zero (s0 = 0: kept), 1 an infinite s0 (kept), 2 one huge negative entry, 3 a NaN
    (every err NaN, index 0), 4 exact at ratios 1 and 0.5 (the first wins), 5 all negative (s0 = 0)."""
    rng = np.random.default_rng(bw)
    w = rng.standard_normal((130, 7)).astype(np.float32)
    w[:, 0] = 0
    w[17, 2] = -3e4
    w[129, 3] = np.nan
    w[:, 4] = rng.integers(-(1 << bw - 2), 1 << bw - 2, 130)  # whole steps of s0 = 1 and of 0.5, in range
    w[:, 5] = -np.abs(w[:, 5])
    s0 = P.column_scales(w, 1, bw)
    s0[1], s0[3], s0[4] = np.inf, 0.125, 1.0
    ratio = np.array([1.0, 0.75, 0.5, 0.875], np.float32)
    got, want = _search(w, s0, ratio, bw), R.search_cols(w, s0, ratio, bw)
    _check(got, want)
    scale, index, err = got
    assert s0[0] == 0 and s0[5] == 0 and index[[0, 1, 3, 4, 5]].tolist() == [0] * 5
    assert np.isinf(scale[1]) and not err[:, [0, 1, 5]].any() and np.signbit(err[:, [0, 1, 5]]).sum() == 0
    assert np.isnan(err[:, 3]).all() and err[0, 4] == 0 and err[2, 4] == 0 and err[1, 4] > 0


def test_kernel_refusals():
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    lib = _lib.load()
    w = DeviceArray.from_host(np.ones((4, 8), np.float32))
    s0, ratio = DeviceArray.from_host(np.ones(8, np.float32)), DeviceArray.from_host(R.ratios(4))
    scale, index = DeviceArray.from_host(np.full(8, 5, np.float32)), DeviceArray((8,), np.int32)
    err = DeviceArray((4, 8), np.float64)
    null, fn = ctypes.c_void_p(0), lib.nqk_clip_search_cols
    good = [w.vp, 4, 8, 8, s0.vp, ratio.vp, 4, 4, scale.vp, index.vp, err.vp]
    for pos, value, word in ((1, 0, b"empty"), (2, 0, b"empty"), (3, 7, b"ld < cols"), (6, 0, b"G must"), (6, 65, b"G must"),
                             (7, 0, b"bit_width"), (7, 9, b"bit_width"), (0, null, b"null"), (4, null, b"null"),
                             (5, null, b"null"), (8, null, b"null"), (9, null, b"null"),
                             (0, ctypes.c_void_p(w.ptr + 2), b"alignment"), (10, ctypes.c_void_p(err.ptr + 4), b"alignment")):
        args = list(good)
        args[pos] = value
        assert fn(*args) != 0, (pos, value)
        assert word in lib.nqk_last_error(), (pos, lib.nqk_last_error())
    assert np.array_equal(scale.to_host(), np.full(8, 5, np.float32))  # nothing above was launched
    good[10] = null  # err may be absent
    assert fn(*good) == 0 and np.array_equal(scale.to_host(), np.ones(8, np.float32))
    for args, kw in (((w, s0, ratio, 9), {}), ((w, s0, R.ratios(65), 4), {}), ((w, np.ones(7, np.float32), ratio, 4), {}),
                     ((w, s0, ratio, 4), dict(rows=5, cols=8, ld=8)), ((w, np.ones(8), ratio, 4), {})):
        with pytest.raises(ValueError):
            K.clip_search_cols(*args, **kw)


# ----------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def graphs():
    """name -> (what Model.from_onnx takes, oracle graph, input, clip_steps): mlp.onnx (Gemm weights
    [N][K], transB: axis 0) at 64 steps, the encoder layer with the per-column tests' spread weights
    at 6; and the restatement's result per (name, bw, per_channel), computed once."""
    from numpy_quant import onnx_proto
    from oracle import nq_oracle as O
    path = os.path.join(MODELS, "mlp.onnx")
    proto, graph, x = M.encoder_layer_fixture(MODELS)
    g = {"mlp": (path, O.Graph(onnx_proto.load(path)), np.random.default_rng(0).uniform(-1.2, 1.2, size=(64, 2)).astype(np.float32), 64),
         "layer": (proto, graph, x, 6)}
    cache = {}

    def ref(name, bw, pc):
        if (name, bw, pc) not in cache:
            _, graph, x, steps = g[name]
            cache[name, bw, pc] = R.calibrate(graph, [x], bw, 4, pc, steps)
        return cache[name, bw, pc]

    return g, ref


@pytest.mark.parametrize("pc", [False, True], ids=["per_tensor", "per_column"])
@pytest.mark.parametrize("bw", [8, 4])
@pytest.mark.parametrize("name", ["mlp", "layer"])
def test_quantize_with_the_search_equals_the_restatements_scales(graphs, name, bw, pc):
    g, ref = graphs
    source, graph, x, steps = g[name]
    qp, qc, axes = ref(name, bw, pc)
    assert axes and (name != "mlp" or set(axes.values()) == {0})
    assert name == "mlp" or any(not np.array_equal(qp[n].scale, M.quantize_weight(graph.constants[n], 4, pc, a)[1])
                                for n, a in axes.items())  # the search moved a scale of the layer
    from numpy_quant.model import Model, QuantizationParams
    model = Model.from_onnx(source)
    given = {k: QuantizationParams(v.scale, v.zero_point) for k, v in qp.items()}
    got = model.quantize([x], bit_width=bw, weight_bit_width=4, per_channel=pc, weight_clip="mse", clip_steps=steps)
    want = model.quantize_with(given, bit_width=bw, weight_bit_width=4, per_channel=pc)
    assert got.weight_clip == "mse" and want.weight_clip is None and got.weight_bit_width == 4
    consts = {v.name: v.data for v in got.values}
    for n in axes:
        s = np.asarray(got.quant_params[n].scale)
        assert s.dtype == np.float32 and s.shape == np.shape(qp[n].scale), n
        assert np.array_equal(s.view(np.uint32), np.asarray(qp[n].scale).view(np.uint32)), n
        assert np.array_equal(consts[n].data, qc[n][1]), n
    for n, p in want.quant_params.items():
        assert np.array_equal(np.asarray(got.quant_params[n].scale), np.asarray(p.scale)), n
    for keep in (True, False):  # the node loop, then the fused plan
        got.keep_values = want.keep_values = keep
        assert np.array_equal(got([x])[0].view(np.uint32), want([x])[0].view(np.uint32))
    assert name != "layer" or (got._plan.fused == 1 and want._plan.fused == 1)


def test_none_is_todays_model_and_the_refusals_come_before_the_forward(graphs):
    from numpy_quant import blob
    from numpy_quant.model import Constant, Model
    source, _, x, _ = graphs[0]["mlp"]
    model = Model.from_onnx(source)
    blobs = []
    for k, kw in enumerate((dict(), dict(weight_clip=None, clip_steps=3))):
        q = model.quantize([x], bit_width=8, weight_bit_width=4, per_channel=True, **kw)
        assert q.weight_clip is None
        consts = [(v.name, v.data.data.tobytes()) for v in q.values if isinstance(v, Constant)]
        blobs.append((json.dumps(blob.pack(q)[0]), consts, q([x])[0].tobytes()))  # the blob's header and every constant
    assert blobs[0] == blobs[1]

    def never():
        raise AssertionError("the calibration forward ran")
        yield

    for kw in (dict(weight_clip="mse", clip_weights=True), dict(weight_clip="abs"), dict(weight_clip="mse", clip_steps=65),
               dict(weight_clip="mse", bit_width=16)):
        with pytest.raises(ValueError):
            model.quantize_stream(never(), **kw)
    for kw in (dict(weight_clip="abs"), dict(weight_clip="mse", clip_steps=0)):
        with pytest.raises(ValueError):
            model.quantize(never(), **kw)
    q = model.quantize_stream([[x]], bit_width=8, weight_bit_width=4, weight_clip="mse")
    assert q.weight_clip == "mse"
