"""The integer Conv's NumPy restatement (tests/_qconv_ref.py) against a brute-force integer
convolution, and its distance to the float Conv on the dequantized operands.  No GPU."""
import numpy as np
import pytest

import _qconv_ref as R
from oracle import nq_oracle as O

PADDED = dict(xs=(2, 3, 7, 9), ws=(4, 3, 3, 2), pads=(0, 2, 2, 1), strides=(2, 1))
PATCH = dict(xs=(2, 3, 32, 48), ws=(8, 3, 16, 16), pads=(0, 0, 0, 0), strides=(16, 16))


def _ints(case, seed, lo=-128, hi=128):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, size=case["xs"], dtype=np.int64), rng.integers(lo, hi, size=case["ws"], dtype=np.int64)


@pytest.mark.parametrize("case", [PADDED, PATCH], ids=["padded", "patchify"])
@pytest.mark.parametrize("zx,zw", [(-7, None), (None, None), (-7, 5), (None, 5)])
def test_restatement_equals_brute_force(case, zx, zw):
    xq, wq = _ints(case, 1)
    got, ho, wo = R.centred(xq, zx, wq, zw, case["pads"], case["strides"])
    want = R.brute(xq, zx, wq, zw, case["pads"], case["strides"])
    assert got.shape == (case["xs"][0] * ho * wo, case["ws"][0])
    np.testing.assert_array_equal(got, want)


def test_padded_cells_hold_the_zero_point():
    xq, _ = _ints(PADDED, 2)
    cols, ho, wo = R.im2col_q(xq, 3, 2, PADDED["pads"], PADDED["strides"], -7)
    assert (ho, wo) == (4, 11)
    # output (oy, ox) = (0, 0): columns kj = 0, 1 sit at ix = -2, -1 — every cell is padding
    np.testing.assert_array_equal(cols[0], np.full(3 * 2 * 3, -7))
    zero, _, _ = R.im2col_q(xq, 3, 2, PADDED["pads"], PADDED["strides"], None)
    np.testing.assert_array_equal(zero[0], np.zeros(18, dtype=np.int64))


@pytest.mark.parametrize("case", [PADDED, PATCH], ids=["padded", "patchify"])
@pytest.mark.parametrize("zx", [-7, None])
def test_close_to_float_conv_by_derived_bound(case, zx):
    """|y_int - y_float| <= (K + 4) 2^-23 sum_k |dx_k dw_k|, the sum in float64: the float Conv
    is an fmaf chain of K products of the dequantized operands (K 2^-24 relative to the sum of
    magnitudes, to first order), plus the roundings of dx, dw, f32(sx sw) and of the result
    (4 x 2^-24); 2^-23 instead of 2^-24 covers the second-order terms."""
    xq, wq = _ints(case, 3)
    sx, sw = np.float32(0.0371), np.float32(0.0042)
    y_int, ho, wo = R.pre_bias(xq, zx, sx, wq, None, sw, case["pads"], case["strides"])
    dx, dw = O.dequantize(xq, sx, zx), O.dequantize(wq, sw, None)
    kout, c, kh, kw = case["ws"]
    y_float = O.conv2d_nchw(dx, dw, np.zeros(kout, np.float32), case["pads"], case["strides"])
    y_float = y_float.transpose(0, 2, 3, 1).reshape(-1, kout)
    # sum_k |dx_k dw_k| per output: the same convolution on the magnitudes (padding is 0.0), in float64
    ph0, pw0, ph1, pw1 = case["pads"]
    sh, sw_ = case["strides"]
    ax = np.pad(np.abs(dx).astype(np.float64), ((0, 0), (0, 0), (ph0, ph1), (pw0, pw1)))
    aw = np.abs(dw).astype(np.float64)
    mag = np.zeros((case["xs"][0], ho, wo, kout))
    for ki in range(kh):
        for kj in range(kw):
            win = ax[:, :, ki:ki + sh * ho:sh, kj:kj + sw_ * wo:sw_][:, :, :ho, :wo]
            mag += np.einsum("bcyx,nc->byxn", win, aw[:, :, ki, kj])
    bound = (kh * kw * c + 4) * 2.0 ** -23 * mag.reshape(-1, kout)
    err = np.abs(y_int.astype(np.float64) - y_float.astype(np.float64))
    assert (err <= bound).all(), float((err - bound).max())
