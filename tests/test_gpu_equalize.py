"""Channel equalization on the GPU: nqk_absmax_f32 against np.abs(x).max(axis) in bits, and
Model.equalize against the NumPy restatement (tests/_equalize_ref.py) bit for bit: the exponents,
the rewritten constants, the float forward, the quantized node loop, the fused plan, a DeviceGraph
replay, the blob, and the other opt-in quantization features beside it."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import ROOT

import _calib_ref as C
import _equalize_ref as R
import _mixed_ref as M
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _data(rng, shape):
    """normal data over many exponents with exact zeros and -0.0"""
    x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-4, 5, shape)).astype(np.float32)
    x[rng.random(shape) < 0.1] = 0.0
    x[rng.random(shape) < 0.02] = -0.0
    return x


def _absmax(x, axis, ld=None, offset=0, state=None):
    """The state after nqk_absmax_f32 on x [rows, cols], stored with row stride ld `offset` floats
    into its buffer; everything around x holds a NaN, which no correct kernel reads."""
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rows, cols = x.shape
    ld = cols if ld is None else ld
    host = np.full(offset + rows * ld + 5, np.nan, np.float32)
    body = host[offset:offset + rows * ld].reshape(rows, ld)
    body[:, :cols] = x
    buf = DeviceArray.from_host(host)
    n = cols if axis == 0 else rows
    if state is None:
        state = DeviceArray((n,), np.uint32).fill_zero()
    K.absmax(buf.offset_view(offset, (rows * ld,)), state, axis, rows=rows, cols=cols, ld=ld)
    return state


# ----------------------------------------------------------------------------- the kernel
# (rows, cols, ld, offset): one element; odd sizes without and with a padded row; three columns (the
# 4-column instance, several row chunks); several workgroups per column with a ragged row chunk and
# a ragged column strip, scalar (ld = 70) and with 16-byte loads (ld = 72); more than one strip of
# 256 columns; a base pointer one, two and three floats off the 16-byte phase (a scalar head and tail)
AXIS0 = [(1, 1, 1, 0), (37, 50, 50, 0), (37, 50, 64, 0), (1000, 3, 3, 0), (4099, 70, 70, 0), (4099, 70, 72, 0),
         (300, 517, 520, 0), (37, 50, 64, 1), (4099, 70, 72, 1), (131, 261, 264, 2), (131, 261, 264, 3),
         (5, 3, 4, 1), (70, 6, 8, 3)]


@pytest.mark.parametrize("rows,cols,ld,offset", AXIS0)
def test_absmax_axis0(rows, cols, ld, offset):
    x = _data(np.random.default_rng(rows * 1000 + cols + offset), (rows, cols))
    got = _absmax(x, 0, ld, offset).to_host()
    assert got.dtype == np.uint32 and np.array_equal(got, _u32(np.abs(x).max(axis=0)))
    assert np.array_equal(got, R.absmax(x, 0).view(np.uint32))


@pytest.mark.parametrize("rows,cols,ld,offset", [(50, 37, 37, 0), (768, 70, 70, 0), (768, 70, 72, 1), (9, 1031, 1032, 0),
                                                 (1, 1, 1, 0), (3000, 2, 2, 1), (5, 1031, 1033, 3)])
def test_absmax_axis1(rows, cols, ld, offset):
    """A wave per row; the rows of the short, wide arrays are cut into segments (ragged last one)."""
    x = _data(np.random.default_rng(rows * 1000 + cols + offset), (rows, cols))
    got = _absmax(x, 1, ld, offset).to_host()
    assert np.array_equal(got, _u32(np.abs(x).max(axis=1)))


@pytest.mark.parametrize("axis", [0, 1])
def test_absmax_two_calls_equal_the_concatenation(axis):
    rng = np.random.default_rng(axis)
    a, b = _data(rng, (150, 70)), _data(rng, (61, 70))
    if axis == 1:
        a, b = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
    state = _absmax(a, axis)
    first = state.to_host()
    both = _absmax(b, axis, state=state).to_host()
    whole = np.concatenate([a, b], axis=axis)
    assert np.array_equal(both, _u32(np.abs(whole).max(axis=axis)))
    assert not np.array_equal(both, first)


@pytest.mark.parametrize("axis", [0, 1])
def test_absmax_special_values(axis):
    """Each in one column (row, for axis 1): a largest magnitude that is negative, only -0.0, a
    subnormal on top, -inf, and NaNs of three payloads, which all give 0x7FC00000."""
    x = np.random.default_rng(5).uniform(-1, 1, size=(70, 8)).astype(np.float32)
    x[33, 0] = -7.5
    x[:, 1] = -0.0
    x[:, 2] = 0.0
    x[40, 2] = -3e-41
    x[2, 3] = -np.inf
    x[69, 4] = np.nan
    x[0, 5] = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    x[1, 6] = np.array([0x7F800001], np.uint32).view(np.float32)[0]
    x[5, 6] = np.inf
    if axis == 1:
        x = np.ascontiguousarray(x.T)
    got = _absmax(x, axis).to_host()
    want = _u32(np.abs(x).max(axis=axis))
    assert list(got[:4]) == [_u32(np.float32(7.5))[()], 0, _u32(np.float32(3e-41))[()], 0x7F800000]
    assert list(got[4:7]) == [0x7FC00000] * 3
    assert np.array_equal(got[:4], want[:4]) and np.array_equal(got[7], want[7])
    assert np.all(np.isnan(got[4:7].view(np.float32))) and np.all(np.isnan(want[4:7].view(np.float32)))


def test_absmax_a_larger_key_stays():
    from numpy_quant.device import DeviceArray
    x = np.random.default_rng(6).uniform(-1, 1, size=(300, 70)).astype(np.float32)
    seed = np.zeros(70, np.uint32)
    seed[::2] = _u32(np.float32(2.0))
    seed[3] = 0x7FC00000
    got = _absmax(x, 0, state=DeviceArray.from_host(seed)).to_host()
    want = np.maximum(seed, _u32(np.abs(x).max(axis=0)))
    assert np.array_equal(got, want) and got[0] == seed[0] and got[3] == 0x7FC00000 and got[1] != 0


def test_absmax_refusals_and_empty_sizes():
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    lib = _lib.load()
    x = DeviceArray.from_host(np.full((4, 8), 3.0, np.float32))
    state = DeviceArray((8,), np.uint32).fill_zero()
    fn = lib.nqk_absmax_f32
    null = ctypes.c_void_p(0)
    for args, word in (((null, 4, 8, 8, 0, state.vp), b"null"), ((x.vp, 4, 8, 8, 0, null), b"null"),
                       ((x.vp, -1, 8, 8, 0, state.vp), b"negative"), ((x.vp, 4, -1, 8, 0, state.vp), b"negative"),
                       ((x.vp, 4, 9, 8, 0, state.vp), b"cols > ld"), ((x.vp, 4, 8, 8, 2, state.vp), b"axis"),
                       ((x.vp, 4, 8, 8, -1, state.vp), b"axis"),
                       ((ctypes.c_void_p(x.ptr + 2), 4, 7, 8, 0, state.vp), b"alignment")):
        assert fn(*args) != 0, args
        assert word in lib.nqk_last_error(), (args, lib.nqk_last_error())
    assert fn(x.vp, 0, 8, 8, 0, state.vp) == 0 and fn(x.vp, 4, 0, 8, 1, state.vp) == 0
    assert not state.to_host().any()  # nothing above was launched
    for bad in (lambda: K.absmax(x, state, 2), lambda: K.absmax(x, DeviceArray((7,), np.uint32), 0),
                lambda: K.absmax(x, DeviceArray((8,), np.int32), 0), lambda: K.absmax(x, state, 0, rows=5, cols=8, ld=8),
                lambda: K.absmax(x, state, 0, rows=4, cols=8, ld=7)):
        with pytest.raises(ValueError):
            bad()
    K.absmax(x, state, 0)
    assert np.array_equal(state.to_host(), np.full(8, _u32(np.float32(3.0))[()], np.uint32))


# ----------------------------------------------------------------------------- the encoder layer
@pytest.fixture(scope="module")
def layer():
    """The outlier fixture, the restatement's equalized graphs and their quantized results, each
    computed once and left unchanged."""
    proto, graph, x, picked = R.outlier_fixture(MODELS)
    with np.errstate(all="ignore"):
        vals = O.float_forward(graph, [x])
    cache = {}

    def eq(pow2=True):
        if ("eq", pow2) not in cache:
            with np.errstate(all="ignore"):
                cache[("eq", pow2)] = R.equalize(graph, [[x]], pow2=pow2)
        return cache[("eq", pow2)]

    def ref(equalized, bw=8, wbw=None, pc=False):
        key = (equalized, bw, wbw, pc)
        if key not in cache:
            g = eq()[0] if equalized else graph
            qp, qc, axes = M.calibrate(g, [x], bw, weight_bit_width=wbw, per_channel=pc)
            v = M.quantized_forward(g, qp, qc, [x], bw, weights=axes)
            cache[key] = (qp, qc, v, M.outputs_of(g, v)[0])
        return cache[key]

    return dict(proto=proto, graph=graph, x=x, picked=picked, vals=vals, eq=eq, ref=ref)


def _model(proto):
    from numpy_quant.model import Model
    return Model.from_onnx(proto)


def _given(qp):
    from numpy_quant.model import QuantizationParams
    return {k: QuantizationParams(v.scale, v.zero_point) for k, v in qp.items()}


def _constants(model):
    from numpy_quant.model import Constant
    return {v.name: v.data.data for v in model.values if isinstance(v, Constant)}


def _digest(model):
    h = hashlib.sha256()
    for name, arr in sorted(_constants(model).items()):
        h.update(name.encode())
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()


def _check_integers(qmodel, vals):
    from numpy_quant.tensor import QTensor
    seen = 0
    for v in qmodel.values:
        t, want = v.data, vals.get(v.name)
        if not isinstance(t, QTensor) or want is None or want[0] != "Q":
            continue
        assert np.array_equal(t.data, want[1]), v.name
        assert np.array_equal(np.asarray(t.scale, np.float32), np.asarray(want[3], np.float32)), v.name
        seen += 1
    assert seen > 20


@pytest.mark.parametrize("pow2", [True, False])
def test_equalize_gives_the_restatements_exponents_and_constants(layer, pow2):
    from numpy_quant.equalize import Equalizer, find_sites
    graph, x = layer["graph"], layer["x"]
    want_graph, want_vec = layer["eq"](pow2)
    model = _model(layer["proto"])
    sites = find_sites(model)
    assert [(s.out, s.gamma, s.beta, s.weights, s.K) for s in sites] == \
        [(s.out, s.gamma, s.beta, s.weights, s.K) for s in R.find_sites(graph)]
    assert [len(s.weights) for s in sites] == [3, 1] and model.equalization is None
    before = _digest(model)
    eqm = model.equalize([[x]], pow2=pow2)
    info = eqm.equalization
    assert [s.out for s in info.sites] == [s.out for s in sites] and info.pow2 == pow2 and info.alpha == 0.5 and info.emax == 8
    for s in info.sites:
        assert s.vector.dtype == (np.int64 if pow2 else np.float64)
        assert np.array_equal(s.vector, want_vec[s.out]), s.out
        if pow2:
            assert np.all(s.vector[layer["picked"][s.out]] >= 2)
            assert np.array_equal(s.scale, np.exp2(s.vector.astype(np.float64)).astype(np.float32))
    got = _constants(eqm)
    assert set(got) == set(want_graph.constants)
    for name, arr in want_graph.constants.items():
        assert np.array_equal(_u32(got[name]), _u32(arr)), name
    # the source is as it was, and what was not rewritten is shared, not copied
    assert _digest(model) == before and _digest(model) != _digest(eqm)
    changed = {n for s in sites for n in (s.gamma, s.beta, *s.weights)}
    src = {v.name: v for v in model.values}
    for v in eqm.values:
        if v.name in got:
            assert (v.data is src[v.name].data) == (v.name not in changed), v.name
        assert v is not src[v.name]
    # the Equalizer in steps: two observations of one batch change nothing (a maximum)
    eq = Equalizer(model, pow2=pow2)
    model._forward([x])
    eq.observe()
    eq.observe()
    vec = eq.exponents()
    assert all(np.array_equal(vec[k], want_vec[k]) for k in want_vec)
    a, w = eq.maxima()[sites[1].out]
    assert np.array_equal(_u32(w), _u32(R.weight_maxima(graph, R.find_sites(graph)[1])))
    assert np.array_equal(_u32(a), _u32(R.activation_maxima(graph, [[x]])[sites[1].out]))


def test_equalized_float_model_is_bit_identical(layer):
    x, vals = layer["x"], layer["vals"]
    model = _model(layer["proto"])
    eqm = model.equalize([[x]])
    want = O.outputs_of(layer["graph"], vals)[0]
    out = eqm([x])[0]
    assert np.array_equal(_u32(out), _u32(want)) and np.array_equal(_u32(model([x])[0]), _u32(want))
    data = {v.name: v.data for v in eqm.values}
    for s in eqm.equalization.sites:
        scaled = vals[s.out][1] * np.exp2(-s.vector).astype(np.float32)
        assert np.array_equal(_u32(data[s.out].data), _u32(scaled)), s.out
    # two batches: the exponents of the restatement over both
    x2 = np.random.default_rng(99).standard_normal(x.shape).astype(np.float32) * np.float32(1.5)
    with np.errstate(all="ignore"):
        want2 = R.exponents(layer["graph"], [[x], [x2]])
    two = model.equalize(([b] for b in (x, x2)))  # a generator: one pass
    assert all(np.array_equal(s.vector, want2[s.out]) for s in two.equalization.sites)
    assert any(not np.array_equal(s.vector, t.vector) for s, t in zip(two.equalization.sites, eqm.equalization.sites))


def test_quantized_8_bit_node_loop_plan_graph_and_blob(layer, tmp_path):
    x = layer["x"]
    qp, qc, vals, want = layer["ref"](True)
    eqm = _model(layer["proto"]).equalize([[x]])
    for qmodel in (eqm.quantize([x], bit_width=8), eqm.quantize_with(_given(qp), bit_width=8)):
        for name, p in qp.items():
            g = qmodel.quant_params[name]
            assert np.float32(g.scale).tobytes() == np.float32(p.scale).tobytes(), name
            assert (g.zero_point is None) == (p.zero_point is None) and (p.zero_point is None or int(g.zero_point) == int(p.zero_point))
        qmodel.keep_values = True
        assert np.array_equal(_u32(qmodel([x])[0]), _u32(want))
        _check_integers(qmodel, vals)
        qmodel.keep_values = False
        plan = qmodel.compile()
        assert plan.fused == 1
        assert np.array_equal(_u32(qmodel([x])[0]), _u32(want))
    g = qmodel.graph([x])
    try:
        assert g.plan.fused == 1
        assert np.array_equal(_u32(g([x])[0]), _u32(want))
        assert np.array_equal(_u32(g([np.ascontiguousarray(x[::-1])])[0]), _u32(want[::-1]))
    finally:
        g.destroy()
    path = str(tmp_path / "eq.nqk")
    qmodel.save(path)
    back = eqm.load_quantized(path)
    assert back.bit_width == 8 and back.equalization is None
    back.keep_values = True
    assert np.array_equal(_u32(back([x])[0]), _u32(want))
    _check_integers(back, vals)
    back.keep_values = False
    assert np.array_equal(_u32(back([x])[0]), _u32(want))
    # the plain model of the same graph still gives the plain restatement
    plain = _model(layer["proto"]).quantize([x], bit_width=8)
    assert np.array_equal(_u32(plain([x])[0]), _u32(layer["ref"](False)[3]))


@pytest.mark.parametrize("kw", [dict(per_channel=True), dict(weight_bit_width=4), dict(integer_conv=True)],
                         ids=["per_channel", "w4a8", "integer_conv"])
def test_other_features_beside_equalization(layer, kw):
    x = layer["x"]
    qp, qc, vals, want = layer["ref"](True, 8, kw.get("weight_bit_width"), kw.get("per_channel", False))
    eqm = _model(layer["proto"]).equalize([[x]])
    qmodel = eqm.quantize([x], bit_width=8, **kw)
    qmodel.keep_values = True
    assert np.array_equal(_u32(qmodel([x])[0]), _u32(want))
    _check_integers(qmodel, vals)
    qmodel.keep_values = False
    assert qmodel.compile().fused == 1
    assert np.array_equal(_u32(qmodel([x])[0]), _u32(want))


def test_quantize_stream_percentile_beside_equalization(layer):
    x = layer["x"]
    want_graph, _ = layer["eq"]()
    eqm = _model(layer["proto"]).equalize([[x]])
    q = eqm.quantize_stream([[x]], bit_width=8, percentile=99.99)
    with np.errstate(all="ignore"):
        fvals = O.float_forward(want_graph, [x])
    for s in eqm.equalization.sites:  # the clipped ranges are those of the restatement's equalized LN outputs
        mn, mx = C.sort_ranges(fvals[s.out][1], 99.99)
        s_ref, z_ref = O.quant_parameters(mn, mx, 8, True)
        p = q.quant_params[s.out]
        assert np.float32(p.scale).tobytes() == np.float32(s_ref).tobytes() and int(p.zero_point) == int(z_ref), s.out
        assert mx < fvals[s.out][1].max()
    qp, qc = O.quantize_with(want_graph, {k: O.QParams(v.scale, v.zero_point) for k, v in q.quant_params.items()}, 8)
    want = M.outputs_of(want_graph, M.quantized_forward(want_graph, qp, qc, [x], 8))[0]
    q.keep_values = True
    assert np.array_equal(_u32(q([x])[0]), _u32(want))
    q.keep_values = False
    assert q.compile().fused == 1 and np.array_equal(_u32(q([x])[0]), _u32(want))


def test_compare_reports_a_lower_8_bit_error(layer):
    x = layer["x"]
    model = _model(layer["proto"])
    eqm = model.equalize([[x]])
    out_name = layer["graph"].outputs[0]
    mse = {}
    for tag, m in (("plain", model), ("equalized", eqm)):
        rep = m.compare(m.quantize([x], bit_width=8), [[x]], k=1)
        mse[tag] = rep.values[out_name].mse
        print(f"8-bit outlier fixture, {tag}: output MSE {mse[tag]:.6g}, SQNR {rep.values[out_name].sqnr_db:.3f} dB")
    assert mse["equalized"] < mse["plain"]
    want = {tag: R.mse(O.outputs_of(layer["graph"], layer["vals"])[0], layer["ref"](tag == "equalized")[3]) for tag in mse}
    # the report's ordered float64 sum and NumPy's pairwise one are each within n 2^-53 = 3.4e-11 of the exact sum
    assert all(abs(mse[t] - want[t]) <= 1e-9 * want[t] for t in mse)


# ----------------------------------------------------------------------------- other graphs
def test_vit_tiny_classifier():
    """ViT-Ti/16 at batch 3: 24 sites with the restatement's exponents, the same plan as the plain
    model (12 fused layers and the CLS tail), plan logits = node loop = the restatement."""
    from numpy_quant import onnx_proto
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
    assert onnx_proto.redimension(proto, 192, 3, 768) > 0
    onnx_proto.rebatch(proto, 3)
    graph = O.Graph(proto)
    x = np.random.default_rng(11).standard_normal((3, 3, 224, 224)).astype(np.float32)
    with np.errstate(all="ignore"):
        want_graph, want_vec = R.equalize(graph, [[x]])
    assert len(want_vec) == 24
    model = _model(proto)
    eqm = model.equalize([[x]])
    sites = eqm.equalization.sites
    assert len(sites) == 24 and [len(s.weights) for s in sites] == [3, 1] * 12 and all(s.K == 192 for s in sites)
    for s in sites:
        assert np.array_equal(s.vector, want_vec[s.out]), s.out
    assert np.array_equal(_u32(eqm([x])[0]), _u32(model([x])[0]))
    qp, qc, axes = M.calibrate(want_graph, [x], 8)
    want = M.outputs_of(want_graph, M.quantized_forward(want_graph, qp, qc, [x], 8))[0]
    plans = {}
    for tag, m in (("plain", model), ("equalized", eqm)):
        q = m.quantize([x], bit_width=8)
        q.keep_values = True
        eager = q([x])[0]
        q.keep_values = False
        plan = q.compile()
        plans[tag] = (plan.embeds, plan.pushdowns, plan.fused, plan.cls_tails)
        assert np.array_equal(_u32(q([x])[0]), _u32(eager)), tag
        if tag == "equalized":
            assert np.array_equal(_u32(eager), _u32(want))
    assert plans["equalized"] == plans["plain"] and plans["plain"][2:] == (12, 1)


def test_graphs_without_a_site():
    from numpy_quant import onnx_proto
    from numpy_quant.equalize import find_sites
    path = os.path.join(MODELS, "mlp.onnx")
    x = np.random.default_rng(0).uniform(-1.2, 1.2, size=(64, 2)).astype(np.float32)
    model = _model(path)
    eqm = model.equalize([[x]])
    assert eqm.equalization is not None and eqm.equalization.sites == []
    a, b = _constants(model), _constants(eqm)
    assert set(a) == set(b) and all(np.array_equal(_u32(a[n]), _u32(b[n])) for n in a)
    assert np.array_equal(_u32(eqm([x])[0]), _u32(model([x])[0]))
    assert np.array_equal(_u32(eqm.quantize([x])([x])[0]), _u32(model.quantize([x])([x])[0]))
    # the encoder layer as shipped: its second LayerNorm takes Identities of the first one's parameters
    layer = onnx_proto.load(os.path.join(MODELS, R.LAYER), synthetic_weights=True)
    assert find_sites(_model(layer)) == [] and R.find_sites(O.Graph(layer)) == []


def test_source_and_result_outlive_each_other(layer):
    x = layer["x"]
    want = O.outputs_of(layer["graph"], layer["vals"])[0]
    model = _model(layer["proto"])
    before = _digest(model)
    eqm = model.equalize([[x]])
    assert _digest(model) == before
    del eqm
    assert np.array_equal(_u32(model([x])[0]), _u32(want)) and _digest(model) == before
    eqm = model.equalize([[x]])
    eq_digest = _digest(eqm)
    del model
    assert np.array_equal(_u32(eqm([x])[0]), _u32(want)) and _digest(eqm) == eq_digest
    assert len(eqm.equalize([[x]]).equalization.sites) == 2  # an equalized model is a Model like any other


def test_bad_arguments(layer):
    x = layer["x"]
    model = _model(layer["proto"])
    for kw in (dict(alpha=1.5), dict(alpha=-0.01), dict(emax=0), dict(emax=17), dict(emax=2.5), dict(alpha="0.5")):
        with pytest.raises(ValueError):
            model.equalize([[x]], **kw)
    with pytest.raises(ValueError):
        model.equalize([])
    with pytest.raises(ValueError):
        model.equalize(iter(()))
    with pytest.raises(ValueError):
        model.quantize([x]).equalize([[x]])
    assert model.equalize([[x]], alpha=0, emax=1).equalization.emax == 1
    assert model.equalize([[x]], alpha=1, emax=16).equalization.alpha == 1.0
