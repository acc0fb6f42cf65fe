"""Host side of the top-k feature: the NumPy reference (_topk_ref.py) against the ordering rule
spelled out as a Python sort, and the argument checks of kernels.topk_softmax, which raise
before the library is loaded (so they run without a GPU)."""
import numpy as np
import pytest

import _topk_ref as R


def _rows():
    rng = np.random.default_rng(7)
    rows = {
        "normal": rng.standard_normal(97).astype(np.float32),
        "four_values": rng.choice(np.array([-1.5, 0.0, 0.25, 3.0], np.float32), size=130),
        "all_equal": np.full(40, 2.5, np.float32),
        "int8_like": (rng.integers(-128, 128, size=1000) * np.float32(0.0371)).astype(np.float32),
        "zeros": np.where(rng.random(70) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
        "zeros_and_negatives": rng.choice(np.array([0.0, -0.0, -1.0], np.float32), size=66),
        "inf": rng.standard_normal(50).astype(np.float32),
        "nan": rng.standard_normal(75).astype(np.float32),
        "all_nan": np.full(9, np.nan, np.float32),
    }
    rows["inf"][[3, 17]] = np.inf
    rows["inf"][[0, 49]] = -np.inf
    rows["nan"][[0, 5, 6, 74]] = np.nan
    rows["nan"][[2, 9]] = np.nanmax(rows["nan"])  # a tie at the top beside the NaNs
    assert np.signbit(rows["zeros"]).any() and not np.signbit(rows["zeros"]).all()
    return rows


@pytest.mark.parametrize("name", sorted(_rows()))
def test_reference_is_the_ordering_rule(name):
    row = _rows()[name]
    n = row.size
    for k in sorted({1, 2, 5, min(n, 64), n}):
        np.testing.assert_array_equal(R.topk_indices(row, k), R.brute_force_indices(row, k), err_msg=f"{name} k={k}")
    idx, prob, value = R.topk_softmax(row[None], min(5, n))
    np.testing.assert_array_equal(R.bits(value[0]), R.bits(row[idx[0]]))
    if name not in ("inf", "nan", "all_nan"):
        full = R.softmax(row)
        assert abs(float(full.sum()) - 1.0) < 1e-5
        np.testing.assert_array_equal(R.bits(prob[0]), R.bits(full[idx[0]]))
        assert np.all(np.diff(prob[0]) <= 0)


def test_reference_rows_have_ties():
    rows = _rows()
    for name in ("four_values", "all_equal", "int8_like", "zeros"):
        top = rows[name][R.topk_indices(rows[name], 5)]
        assert np.unique(top).size < 5, name
    # -0.0 and +0.0 tie: the first five columns, whatever their signs
    np.testing.assert_array_equal(R.topk_indices(rows["zeros"], 5), np.arange(5))
    # NaNs come last, in column order
    np.testing.assert_array_equal(R.topk_indices(rows["nan"], 75)[-4:], [0, 5, 6, 74])


def test_reference_dequantize():
    q = np.array([-128, -1, 0, 5, 127], np.int64)
    s = np.float32(0.0123)
    want = ((q - 3).astype(np.float64) * np.float64(s)).astype(np.float32)
    np.testing.assert_array_equal(R.bits(R.dequantize(q.astype(np.int8), s, 3)), R.bits(want))
    np.testing.assert_array_equal(R.bits(R.dequantize(q, s, None)),
                                  R.bits((q.astype(np.float64) * np.float64(s)).astype(np.float32)))
    from oracle import nq_oracle as O
    np.testing.assert_array_equal(R.bits(R.dequantize(q, s, 3)), R.bits(O.dequantize(q, s, np.int64(3))))


class _NoBlock:
    """Stands in for a device block: a DeviceArray built on it never allocates"""
    ptr = 0
    size = 0


def _fake(shape, dtype):
    from numpy_quant.device import DeviceArray
    return DeviceArray(shape, dtype, block=_NoBlock(), ptr=0)


def test_argument_checks_raise_before_the_library_is_touched(monkeypatch):
    from numpy_quant import _lib
    from numpy_quant import kernels as K

    def touched(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "ensure_init", touched)
    f = _fake((3, 1000), np.float32)
    q = _fake((3, 1000), np.int8)
    for k in (0, -1, 65, 1001):
        with pytest.raises(ValueError, match="k = "):
            K.topk_softmax(f, k)
    with pytest.raises(ValueError, match="k = 6"):
        K.topk_softmax(_fake((2, 5), np.float32), 6)  # k > cols
    with pytest.raises(ValueError, match="k = 65"):
        K.topk_softmax(_fake((2, 100), np.int8), 65, scale=np.float32(0.5))
    with pytest.raises(ValueError, match="8193"):
        K.topk_softmax(_fake((2, 8193), np.float32), 5)
    with pytest.raises(ValueError, match="float64"):
        K.topk_softmax(_fake((3, 1000), np.float64), 5)
    with pytest.raises(ValueError, match="uint8"):
        K.topk_softmax(_fake((3, 1000), np.uint8), 5)
    zt = K.ZpTerm(_lib.ZP_ROW, 1, 2, 8, None, None, [1, 1, 0, 1, 0], (), (), 3, 1000)
    with pytest.raises(ValueError, match="ZpTerm"):
        K.topk_softmax(_fake((3, 1000), np.int32), 5, scale=np.float32(0.5), zp=zt)
    with pytest.raises(ValueError, match="scalar"):
        K.topk_softmax(q, 5, scale=np.float32(0.5), zp=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="scale"):
        K.topk_softmax(q, 5)  # integer storage without its scale
    with pytest.raises(ValueError, match="integer input only"):
        K.topk_softmax(f, 5, scale=np.float32(0.5))
    with pytest.raises(ValueError, match="integer"):
        K.topk_softmax(f, 2.0)
    with pytest.raises(ValueError, match="at least one axis"):
        K.topk_softmax(_fake((), np.float32), 1)


def test_tensor_topk_refusals_on_the_host(monkeypatch):
    """QTensor.topk: the pending-bias error of dequantize, and a ZpTerm, without a launch"""
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.tensor import QTensor

    def touched(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(_lib, "call", touched)
    acc = _fake((3, 10), np.int32)
    zt = K.ZpTerm(_lib.ZP_ROW, 1, 2, 8, None, None, [1, 1, 0, 1, 0], (), (), 3, 10)
    with pytest.raises(ValueError, match="ZpTerm"):
        QTensor(acc, 32, np.float32(0.5), zt).topk(2)
    bias = QTensor(_fake((10,), np.int32), 32, np.float32(0.5))
    biased = QTensor(acc, 32, np.float32(0.5), np.int64(1)) + bias
    with pytest.raises(ValueError, match="biased Gemm accumulator") as e1:
        biased.topk(2)
    with pytest.raises(ValueError) as e2:
        biased.dequantize()
    assert str(e1.value) == str(e2.value)
