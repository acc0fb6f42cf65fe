"""No GPU: the NumPy statement of nqk_compare_stats (_compare_ref.py) checked on its own, the
package's restatement of it, the derived metrics, and the argument checks of compare_stats /
Comparator / Model.compare / sweep, which raise before the library is touched."""
import math
import os

import numpy as np
import pytest

import _compare_ref as R
from conftest import GOLDEN, ROOT

MLP = os.path.join(ROOT, "numpy-quant_amd", "models", "mlp.onnx")
SIZES = [n for n in R.SIZES if n]


def _bits(s):
    return [int(v) for v in np.asarray(s, dtype=np.int64)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("data", [R.wide, R.narrow])
def test_sums_within_the_a_priori_bound_of_fsum(n, data):
    """n - 1 additions of non-negative terms in any order: within (n - 1) * 2^-53 relative"""
    x, y = data(n)
    s = R.state(x, y).view(np.float64)
    _, ad, dd, xx = R.terms(x, y)
    worst = 0.0
    for w, t in zip((2, 3, 4), (ad, dd, xx)):
        exact = math.fsum(t.tolist())
        err = abs(float(s[w]) - exact) / exact if exact else abs(float(s[w]))
        worst = max(worst, err)
        assert err <= (n - 1) * 2.0 ** -53, (w, err)
    print(f"n = {n}: worst relative error against fsum {worst:.3g}")


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 1024])
def test_narrow_data_tells_the_orders_apart(n):
    """a kernel that summed in index order, or as np.sum does, would not reproduce the state"""
    x, y = R.narrow(n)
    got = R.state(x, y).view(np.float64)[3]
    dd = R.terms(x, y)[2]
    assert got.tobytes() != np.float64(np.sum(dd)).tobytes()
    assert got.tobytes() != np.float64(np.cumsum(dd)[-1]).tobytes()


def test_package_statement_equals_the_independent_one():
    from numpy_quant import compare as C
    assert (C.CMP_STATE, C.CMP_CHUNK) == (R.WORDS, R.CHUNK)
    for n in (0, 1, 5, 1025, 4097, 2 * 4096 + 17, 300 * 4096 + 5):
        for data in (R.wide, R.narrow):
            x, y = data(n, seed=3)
            assert _bits(C.host_state(x, y)) == _bits(R.state(x, y)), n
    a, b = R.wide(5000, seed=1), R.narrow(9000, seed=2)
    assert _bits(C.host_state(*b, state=C.host_state(*a))) == _bits(R.state_of_calls([a, b]))


def test_specials_are_skipped_and_counted():
    x, y = R.narrow(4100, seed=5)
    x, y = x.copy(), y.copy()
    x[[0, 7]] = np.nan
    y[[7, 9]] = np.inf
    x[4099] = -np.inf
    keep = np.ones(4100, bool)
    keep[[0, 7, 9, 4099]] = False
    s = R.state(x, y)
    assert (int(s[0]), int(s[1])) == (4096, 4)
    xz, yz = np.where(keep, x, 0).astype(np.float32), np.where(keep, y, 0).astype(np.float32)
    want = R.state(xz, yz)  # a skipped pair adds what a pair of zeros adds: nothing
    assert _bits(s[2:]) == _bits(want[2:])
    assert int(s[6]) == 0 and int(s[7]) == 0
    m = R.metrics(s)
    assert m["nonfinite"] == 4 and math.isfinite(m["mean_abs"]) and math.isfinite(m["max_abs"])


def test_zero_difference_and_empty_states():
    x, _ = R.wide(5000, seed=6)
    m = R.metrics(R.state(x, x))
    assert m["sqnr_db"] == math.inf and m["mse"] == 0.0 and m["max_abs"] == 0.0 and m["mean_abs"] == 0.0
    z = np.zeros(10, np.float32)
    assert math.isnan(R.metrics(R.state(z, z))["sqnr_db"])
    assert R.metrics(R.state(z, z + 1))["sqnr_db"] == -math.inf
    empty = R.metrics(R.state(z[:0], z[:0]))
    assert empty["count"] == 0 and math.isnan(empty["mean_abs"]) and math.isnan(empty["sqnr_db"])


def test_metrics_are_derived_correctly():
    from numpy_quant import compare as C
    x, y = R.narrow(3000, seed=7)
    x = x.copy()
    x[5] = np.nan
    s = R.state(x, y)
    ok = np.isfinite(x)
    d = x[ok].astype(np.float64) - y[ok].astype(np.float64)
    m = R.metrics(s)
    assert m["count"] == 2999 and m["nonfinite"] == 1
    np.testing.assert_allclose(m["mean_abs"], np.abs(d).mean(), rtol=1e-13)
    np.testing.assert_allclose(m["mse"], (d * d).mean(), rtol=1e-13)
    np.testing.assert_allclose(m["rms_ref"], np.sqrt((x[ok].astype(np.float64) ** 2).mean()), rtol=1e-13)
    np.testing.assert_allclose(m["sqnr_db"], 10 * np.log10((x[ok].astype(np.float64) ** 2).sum() / (d * d).sum()),
                               rtol=1e-12)
    assert m["max_abs"] == np.abs(d).max()
    got = C.stats_from_state(s, "constant", "Initializer")
    for key, val in m.items():
        assert getattr(got, key) == val, key
    assert (got.kind, got.op) == ("constant", "Initializer")
    with pytest.raises(ValueError, match="state"):
        C.stats_from_state(np.zeros(7, np.int64))
    with pytest.raises(ValueError, match="state"):
        C.stats_from_state(np.zeros(8, np.float64))


def test_report_orders_and_serialises():
    import json
    from numpy_quant import compare as C
    ag = C.Agreement(labelled=True)
    f = np.array([[1, 0], [0, 1], [1, 0], [0, 1]])
    q = np.array([[1, 0], [1, 0], [0, 1], [0, 1]])
    ag.add(f, q, np.array([1, 0, 1, 1]))
    x, y = R.narrow(100, seed=8)
    vals = {"exact": C.stats_from_state(R.state(x, x)), "rough": C.stats_from_state(R.state(x, y)),
            "fine": C.stats_from_state(R.state(x, (x + np.float32(1e-3)).astype(np.float32))),
            "void": C.stats_from_state(R.state(x[:0], x[:0]))}
    rep = C.Report(vals, 2, ag, bit_width=4)
    assert (rep.rows, rep.top1_agreement, rep.topk_agreement) == (4, 0.5, 1.0)
    assert rep.top1_accuracy == {"float": 0.75, "quantized": 0.25}
    assert rep.topk_accuracy == {"float": 1.0, "quantized": 1.0}
    assert [n for n, _ in rep.worst(4)] == ["rough", "fine", "exact", "void"]
    assert [n for n, _ in rep.worst(1)] == ["rough"]
    text = str(rep)
    assert all(n in text for n in vals)
    back = json.loads(json.dumps(rep.to_dict()))
    assert back["values"]["rough"]["count"] == 100 and back["top1_agreement"] == 0.5 and back["bit_width"] == 4
    with pytest.raises(ValueError, match="labels"):
        C.Agreement(True).add(f, q, np.array([1, 0, 0]))


# ----------------------------------------------------------------------------- refusals
class _NoBlock:
    ptr = 0
    size = 1 << 40


def _fake(shape, dtype, ptr=0):
    from numpy_quant.device import DeviceArray
    return DeviceArray(shape, dtype, block=_NoBlock(), ptr=ptr)


@pytest.fixture
def untouched(monkeypatch):
    from numpy_quant import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "ensure_init", touched)


def test_compare_stats_refuses_before_the_library_is_touched(untouched):
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    f, q, st = _fake((3, 100), np.float32), _fake((3, 100), np.int8), _fake((8,), np.int64)
    zt = K.ZpTerm(_lib.ZP_ROW, 1, 2, 8, None, None, [1, 1, 0, 1, 0], (), (), 3, 100)
    with pytest.raises(ValueError, match="ZpTerm"):
        K.compare_stats(f, _fake((3, 100), np.int32), st, scale=np.float32(0.5), zp=zt)
    with pytest.raises(ValueError, match="shapes differ"):
        K.compare_stats(f, _fake((100, 3), np.float32), st)
    with pytest.raises(ValueError, match="shapes differ"):
        K.compare_stats(f, _fake((3, 99), np.int8), st, scale=np.float32(0.5))
    for bad in (np.float64, np.uint8, np.float16):
        with pytest.raises(ValueError, match="not supported"):
            K.compare_stats(f, _fake((3, 100), bad), st)
    with pytest.raises(ValueError, match="x must be float32"):
        K.compare_stats(q, f, st)
    with pytest.raises(ValueError, match="needs its scale"):
        K.compare_stats(f, q, st)
    with pytest.raises(ValueError, match="integer y only"):
        K.compare_stats(f, f, st, scale=np.float32(0.5))
    with pytest.raises(ValueError, match="scalar"):
        K.compare_stats(f, q, st, scale=np.float32(0.5), zp=np.zeros(3, np.int64))
    for bad in (_fake((7,), np.int64), _fake((8,), np.int32), _fake((1, 8), np.int64)):
        with pytest.raises(ValueError, match="state"):
            K.compare_stats(f, f, bad)
    with pytest.raises(ValueError, match="DeviceArrays"):
        K.compare_stats(np.zeros((3, 100), np.float32), f, st)
    with pytest.raises(ValueError, match="alignment"):
        K.compare_stats(_fake((3, 100), np.float32, ptr=2), f, st)
    with pytest.raises(ValueError, match="alignment"):
        K.compare_stats(f, _fake((3, 100), np.int16, ptr=1), st, scale=np.float32(0.5))
    with pytest.raises(ValueError, match="more than"):
        K.compare_stats(_fake((K.CMP_MAX_N + 1,), np.float32), _fake((K.CMP_MAX_N + 1,), np.float32), st)


def test_comparator_refuses_before_the_library_is_touched(untouched):
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.compare import Comparator
    from numpy_quant.tensor import FTensor, ITensor, QTensor
    cmp = Comparator()
    f = FTensor(_fake((3, 10), np.float32))
    with pytest.raises(ValueError, match="shapes differ"):
        cmp.observe_pair("v", f, FTensor(_fake((10, 3), np.float32)))
    with pytest.raises(ValueError, match="shapes differ"):
        cmp.observe_pair("v", f, QTensor(_fake((3, 11), np.int8), 8, np.float32(0.5)))
    with pytest.raises(ValueError, match="reference side"):
        cmp.observe_pair("v", QTensor(_fake((3, 10), np.int8), 8, np.float32(0.5)), f)
    with pytest.raises(ValueError, match="compared side"):
        cmp.observe_pair("v", f, ITensor(np.zeros((3, 10), np.int64)))
    bias = QTensor(_fake((10,), np.int32), 32, np.float32(0.5))
    biased = QTensor(_fake((3, 10), np.int32), 32, np.float32(0.5), np.int64(1)) + bias
    with pytest.raises(ValueError) as e1:
        cmp.observe_pair("v", f, biased)
    with pytest.raises(ValueError) as e2:
        biased.dequantize()
    assert str(e1.value) == str(e2.value)
    assert cmp.report() == {}
    with pytest.raises(KeyError):
        cmp.state("v")


def test_model_compare_and_sweep_refuse_before_the_library_is_touched(untouched):
    from numpy_quant import compare as C
    from numpy_quant.model import Model, QModel
    model = Model([], [], [], [])
    qmodel = QModel([], [], [], [], 8, {})
    with pytest.raises(ValueError, match="no evaluation batch"):
        model.compare(qmodel, [])
    with pytest.raises(ValueError, match="no evaluation batch"):
        model.compare(qmodel, iter(()), values=False)
    with pytest.raises(ValueError, match="float Model"):
        model.compare(model, [[np.zeros((1, 2), np.float32)]])
    with pytest.raises(ValueError, match="float Model"):
        qmodel.compare(qmodel, [[np.zeros((1, 2), np.float32)]])
    for k in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            model.compare(qmodel, [[np.zeros((1, 2), np.float32)]], k=k)
    batches = [[np.zeros((1, 2), np.float32)]]
    with pytest.raises(ValueError, match="one-pass"):
        C.sweep(model, (b for b in batches), batches)
    with pytest.raises(ValueError, match="one-pass"):
        C.sweep(model, batches, iter(batches))
    with pytest.raises(ValueError, match="one-pass"):
        C.sweep(model, batches, batches, labels=iter([np.zeros(1, np.int64)]))
    with pytest.raises(ValueError, match="bit width"):
        C.sweep(model, batches, batches, bit_widths=())
    for bw in (0, 17, 4.0):
        with pytest.raises(ValueError, match="bit widths"):
            C.sweep(model, batches, batches, bit_widths=(8, bw))
    with pytest.raises(ValueError, match="percentile"):
        C.sweep(model, batches, batches, percentile=40.0)


# ----------------------------------------------------------------------------- the oracle
def oracle_output_mse(bit_width, X):
    """MSE of the quantized MLP's output against the float output, both through the oracle"""
    from numpy_quant import onnx_proto
    from oracle import nq_oracle as O
    graph = O.Graph(onnx_proto.load(MLP))
    want = O.outputs_of(graph, O.float_forward(graph, [X]))[0]
    qp, qc = O.calibrate(graph, [X], bit_width)
    got = O.outputs_of(graph, O.quantized_forward(graph, qp, qc, [X], bit_width))[0]
    d = np.asarray(want, np.float64) - np.asarray(got, np.float64)
    return float((d * d).mean())


def test_oracle_mlp_loses_more_at_4_bits_than_at_8():
    X = np.load(os.path.join(GOLDEN, "mlp.npz"))["X"]
    mse8, mse4 = oracle_output_mse(8, X), oracle_output_mse(4, X)
    print(f"oracle MLP output MSE: 8 bits {mse8:.4g}, 4 bits {mse4:.4g}")
    assert mse4 >= mse8
