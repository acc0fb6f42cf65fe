"""tests/_per_token_ref.py's operand builders, without a GPU: what the near-limit operands of the
row-scaled GEMM must keep true to tell a kernel that rounds P - z colsum through float32, or wraps
it, from one that does not; that the ordinary operands cannot; and what the quantizer's edge rows
give in the restatement."""
import numpy as np
import pytest

import _per_token_ref as R
from oracle import nq_oracle as O


def _f32_exact(v):
    return v.astype(np.float32).astype(np.int64) == v


def _through_f32(v, s, sw):
    """rows_matmul's scaling on the float32 image of the integer: v_cvt_f32_i32 in v_cvt_f64_i32's place."""
    sc = (s[:, None] * sw[None, :]).astype(np.float64)
    return (v.astype(np.float32).astype(np.float64) * sc).astype(np.float32)


@pytest.mark.parametrize("M,N,K", [(1, 1, 16), (127, 129, 80), (129, 160, 768)])
def test_existing_operands_never_leave_float32(M, N, K):
    """Why near_limit_operands exists: P - z colsum of gemm_operands stays below 2^24."""
    a, w, z, s, sw = R.gemm_operands(M, N, K)
    v = R.integers(a, w, z)[1]
    assert np.abs(v).max() < 2 ** 24 and np.all(_f32_exact(v))
    assert np.array_equal(_through_f32(v, s, sw), R.rows_matmul(a, w, s, z, sw))


def test_near_limit_operands_discriminate():
    M, N, K = 40, 48, 65520  # the largest K nqk_qgemm_rows accepts
    a, w, z, s, sw = R.near_limit_operands(M, N, K)
    assert a.shape == (M, K) and w.shape == (K, N) and a.dtype == w.dtype == np.int8
    assert np.all(z[:-1] == 127) and z[-1] == -128 and a[-1].min() >= 100 and a[:-1].max() < -100
    P, v = R.integers(a, w, z)
    assert -2 ** 31 <= v.min() and v.max() < 2 ** 31 and np.abs(P).max() < 2 ** 31  # int32, as the kernel header states
    assert np.abs(v).min() > 2 ** 30 and (v > 0).any() and (v < 0).any()
    inexact = 1 - _f32_exact(v).mean()
    want = R.rows_matmul(a, w, s, z, sw)
    differ = (_through_f32(v, s, sw).view(np.uint32) != want.view(np.uint32)).mean()
    print(f"K={K}: P - z colsum in {v.min()}..{v.max()}, |P| <= {np.abs(P).max()}, {inexact:.1%} not float32, "
          f"f32-rounded restatement differs in {differ:.1%} of the outputs")
    assert inexact >= 0.5 and differ >= 1 / 20 and np.isfinite(want).all()


def test_extreme_scales_reach_every_regime():
    a, w, z, _, _ = R.gemm_operands(33, 48, 96)
    s, sw = R.extreme_scales(33, 48)
    with np.errstate(over="ignore", under="ignore"):
        sc = s[:, None] * sw[None, :]
        out = R.rows_matmul(a, w, s, z, sw)
    tiny = np.finfo(np.float32).tiny
    assert np.isfinite(sc).all() and (sc == 0).any() and ((sc != 0) & (sc < tiny)).any() and (sc == 2.0 ** 127).any()
    assert not np.isnan(out).any() and np.isinf(out).any() and (out == 0).sum() >= (sc == 0).sum()
    assert ((out != 0) & (np.abs(out) < tiny)).any() and (np.isfinite(out) & (np.abs(out) >= tiny)).any()


@pytest.mark.parametrize("cols,long_path", [(257, False), (1021, False), (4095, False), (4100, True), (8195, True)])
def test_extreme_positions_decide_the_scale(cols, long_path):
    """Every row's range is set by its one outlier: a kernel that misses the element at that
    position returns a scale 500 times too small."""
    x, pos = R.extreme_positions(cols, long_path)
    assert {0, 3, 4, 255, 256, cols - 1} <= set(pos) and set(range(0, cols, 256)) <= set(pos)
    assert not long_path or {1023, 1024} <= set(pos)
    q, s, z = R.quantize_rows(x, 8)
    P = len(pos)
    for i, p in enumerate(pos):
        assert x[i, p] == 1000 and x[P + i, p] == -1000 and np.abs(np.delete(x[i], p)).max() <= 1
        assert s[i] > 3.9 and s[P + i] > 3.9 and q[i, p] == 127 and q[P + i, p] == -128
    y = x.copy()
    y[0, pos[0]] = 0  # without the outlier
    assert R.quantize_rows(y[:1], 8)[1][0] < 0.01


def test_range_extremes_in_the_restatement():
    x = R.range_extremes()
    assert x.shape == (6, 70) and np.isfinite(x).all()
    for bw in (8, 4, 2):
        qlo, qhi = (int(v) for v in O.qrange(bw))
        with np.errstate(over="ignore"):
            q, s, z = R.quantize_rows(x, bw)
        assert q.min() >= qlo and q.max() <= qhi and z.min() >= qlo and z.max() <= qhi
        assert np.isinf(s[0]) and z[0] == qlo and np.all(q[0] == qlo)         # hi - lo overflows
        assert np.isfinite(s[1:]).all() and z[1] == qlo and q[1, 0] == qhi   # FLT_MAX
        assert 0 < s[2] < np.finfo(np.float32).tiny and 0 < s[4] and q[4].min() == qlo and q[4].max() >= qhi - 1
        assert (s[5], z[5]) == (1, 0) and not q[5].any()                     # -0.0 and +0.0: degenerate
    s8, s4 = R.quantize_rows(x, 8)[1], R.quantize_rows(x[1:], 4)[1]
    assert s8[2] == np.float32(3e-45) and s8[3] == 1 and s4[2] == np.float32(1e-45)  # underflows at 8 bits only
