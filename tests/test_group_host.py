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
