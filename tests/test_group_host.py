"""tests/_group_ref.py, the restatement of group-wise weight scales, against a plain float64
evaluation of sum_k s_a S[k // g, n] (a - zpa) b at the GPU test's shapes.  The restatement rounds
twice in float32, sg = f32(s_a * S) and the result, 2^-24 relative each; the bound has a factor 2 of
slack and the f64 additions are negligible beside it: |out - ref| <= 2^-22 sum_j |sg P_j|."""
import numpy as np
import pytest

import _group_ref as R


@pytest.mark.parametrize("zpa", R.ZPS)
@pytest.mark.parametrize("M,N,K,g", R.SHAPES)
def test_restatement_against_float64(M, N, K, g, zpa):
    a, b, S = R.operands(M, N, K, g)
    s_a = np.float32(0.0123)
    sg = (s_a * S).astype(np.float32)
    out = R.group_matmul(a, b, sg, zpa, g)
    assert out.dtype == np.float32 and out.shape == (M, N)
    z = 0 if zpa is None else zpa
    w = np.float64(s_a) * np.repeat(S.astype(np.float64), g, axis=0) * b.astype(np.float64)
    ref = (a.astype(np.float64) - z) @ w
    bound = 2.0 ** -22 * np.abs(sg.astype(np.float64)[:, None, :] * R.group_products(a, b, zpa, g)).sum(axis=0)
    err = np.abs(out.astype(np.float64) - ref)
    print(f"M={M} N={N} K={K} g={g} zpa={zpa}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound)
    assert np.count_nonzero(out) > out.size // 2


def _f32_exact(v):
    return v.astype(np.float32).astype(np.float64) == v


def _matmul_through_f32(P, sg):
    """group_matmul with every P_j rounded to float32 first: what a kernel computes that converts
    the int32 partial sum with v_cvt_f32_i32, or multiplies on a float32 image of it."""
    acc = np.zeros(P.shape[1:], np.float64)
    for j in range(P.shape[0]):
        acc = acc + sg[j].astype(np.float64) * P[j].astype(np.float32).astype(np.float64)
    return acc.astype(np.float32)


def test_existing_operands_never_leave_float32():
    """Why near_limit_operands exists: every P_j of SHAPES x ZPS, and of the saturating GPU test,
    is a float32 value, so those tests cannot tell f64(P_j) from f64(f32(P_j))."""
    for M, N, K, g in R.SHAPES:
        a, b, sg = R.operands(M, N, K, g)
        for zpa in R.ZPS:
            P = R.group_products(a, b, zpa, g)
            assert np.all(_f32_exact(P)) and np.array_equal(_matmul_through_f32(P, sg), R.group_matmul(a, b, sg, zpa, g))
    assert _f32_exact(np.float64(255 * 128 * 256))


@pytest.mark.parametrize("M,N,g,frac", [(40, 48, 16384, 0.5), (130, 131, 4096, 0.5)])
def test_near_limit_operands_discriminate(M, N, g, frac):
    a, b, sg = R.near_limit_operands(M, N, g)
    assert a.shape == (M, 2 * g) and b.shape == (2 * g, N) and sg.shape == (2, N) and sg.dtype == np.float32
    P = R.group_products(a, b, 127, g)
    assert np.abs(P).max() < 2.0 ** 29 and np.abs(P).max() <= 255 * 128 * g  # the kernel header's bound
    assert np.all(P[0] > 0) and np.all(P[1] < 0)
    inexact = 1 - _f32_exact(P).mean()
    differ = (_matmul_through_f32(P, sg).view(np.uint32) != R.group_matmul(a, b, sg, 127, g).view(np.uint32)).mean()
    print(f"g={g}: |P_j| in 2^{np.log2(np.abs(P).min()):.3f}..2^{np.log2(np.abs(P).max()):.3f}, "
          f"{inexact:.1%} not float32, f32-rounded restatement differs in {differ:.1%} of the outputs")
    assert inexact >= frac and differ >= 1 / 20


def test_many_groups_depend_on_the_order_of_addition():
    a, b, sg = R.many_group_operands(70, 136)
    for zpa in (None, 127):
        P = R.group_products(a, b, zpa, 32)
        assert P.shape[0] == 64 and np.array_equal(P[32], -P[0])
        acc = np.zeros(P.shape[1:], np.float64)
        for j in reversed(range(64)):
            acc = acc + sg[j].astype(np.float64) * P[j]
        want = R.group_matmul(a, b, sg, zpa, 32)
        differ = (acc.astype(np.float32).view(np.uint32) != want.view(np.uint32)).mean()
        print(f"zpa={zpa}: the groups added in reverse change {differ:.1%} of the outputs")
        assert differ >= 0.5 and np.isfinite(want).all() and np.count_nonzero(want) > want.size // 2


def test_extreme_scales_reach_every_regime():
    a, b, _ = R.operands(33, 48, 96, 32)
    with np.errstate(over="ignore", under="ignore"):
        out = R.group_matmul(a, b, R.extreme_scale_rows(48), 5, 32)
    tiny = np.finfo(np.float32).tiny
    sub = (out != 0) & (np.abs(out) < tiny)
    assert not np.isnan(out).any()
    assert sub[:, 0::5].all() and np.isinf(out[:, 3::5]).any() and (np.abs(out[:, 4::5]) >= tiny).all()
    assert np.isfinite(out[:, [c for c in range(48) if c % 5 != 3]]).all()


def test_scale_rule_and_integers():
    w = (np.random.default_rng(1).standard_normal((64, 5)) * 3).astype(np.float32)
    w[32:, 2] = 0.0                        # an all-zero group: scale 0
    w[:32, 3] = -np.abs(w[:32, 3]) - 1.0   # a negative-only group: range clamped to include 0
    S = R.group_scales(w, 32, 4)
    assert S.shape == (2, 5) and S.dtype == np.float32 and S[1, 2] == 0 and S[0, 3] == 0
    assert S[0, 0] == np.float32(2 * max(w[:32, 0].max(), 0)) / np.float32(15.0)
    q = R.quantize_group(w, S, 32, 4)
    assert q[:, :2].min() >= -8 and q.max() == 7 and np.all(q[:32, 3] == -8)
    assert np.all(q[32:, 2] == -(1 << 63))  # 0 / 0, as an all-zero column of a per-column weight
