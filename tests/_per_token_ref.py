"""NumPy restatement of per-token activation scales (QModel.per_token): the specification.

Row m of a float32 x [rows, K] takes the asymmetric parameters of its own range clamped to include
0 (quant_parameters, float32 scalar arithmetic), and quantize's zero-point formula with them; a row
whose float32 scale is 0 is degenerate: s = 1, z = 0, every q = 0.  The product with a symmetric
weight w [K, N] whose column scales are sw [N]:
    P = sum_k q[m, k] w[k, n]                                   exact
    out[m, n] = f32(f64(P - z[m] colsum[n]) * f64(f32(s[m] * sw[n])))
Nothing here imports numpy_quant.
"""
import numpy as np

from oracle import nq_oracle as O


def quantize_rows(x, bit_width):
    """(q int64 [rows, K], s float32 [rows], z int64 [rows]) of float32 x [rows, K]."""
    assert x.dtype == np.float32 and x.ndim == 2
    zero = np.float32(0)
    q = np.zeros(x.shape, np.int64)
    s, z = np.ones(x.shape[0], np.float32), np.zeros(x.shape[0], np.int64)
    for m, row in enumerate(x):
        lo, hi = np.minimum(row.min(), zero), np.maximum(row.max(), zero)
        if np.float32((hi - lo) / np.float32(2.0 ** bit_width - 1)) == 0:
            continue  # degenerate: s = 1, z = 0, q = 0
        sm, zm = O.quant_parameters(lo, hi, bit_width, True)
        s[m], z[m] = sm, zm
        q[m] = O.quantize(row, bit_width, s[m], np.int64(zm))
    return q, s, z


def rows_matmul(q, w, s, z, sw):
    """float32 [rows, N] of integer q [rows, K], w [K, N], the rows' s, z and float32 sw [N]."""
    assert s.dtype == np.float32 and sw.dtype == np.float32
    w = w.astype(np.int64)
    v = np.matmul(q.astype(np.int64), w) - z.astype(np.int64)[:, None] * w.sum(axis=0)[None, :]
    sc = s[:, None] * sw[None, :]
    assert sc.dtype == np.float32
    return (v.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)


def row_cases(cols, bit_width, seed=0):
    """float32 [5, cols]: an all-zero row, an all-positive and an all-negative row (the clamp to 0
    acts), a row with one entry 1000 times the rest, and a row whose range is (2^bw - 1) / 2 exactly,
    so s = 0.5 and z = -1, filled with (n + 0.5) / 2: every x / s is an exact half."""
    rng = np.random.default_rng(seed + 131 * cols + bit_width)
    qlo, qhi = O.qrange(bit_width)
    x = np.zeros((5, cols), np.float32)
    x[1] = rng.uniform(0.5, 2.0, cols)
    x[2] = -rng.uniform(0.5, 2.0, cols)
    x[3] = rng.standard_normal(cols)
    x[3, cols // 2] *= 1000
    x[4] = (rng.integers(int(qlo) + 1, int(qhi), cols) + 0.5) / 2
    x[4, :2] = [(qlo + 1) / 2, (qhi + 1) / 2][:cols]
    return x


def gemm_operands(M, N, K, seed=0):
    """int8 a [M, K] and w [K, N] over the full range with -128 and 127 present, z int64 [M] drawn
    from {-128, 0, 127, random}, s [M] and sw [N] positive float32, log-uniform over 2^-12..2^4."""
    rng = np.random.default_rng(seed + 1000 * M + 10 * N + K)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    w = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    a[0, 0], a[-1, -1], w[0, 0], w[-1, -1] = -128, 127, 127, -128
    z = np.where(rng.random(M) < 0.25, rng.integers(-128, 128, M), rng.choice([-128, 0, 127], M)).astype(np.int64)
    s = np.exp2(rng.uniform(-12, 4, M)).astype(np.float32)
    return a, w, z, s, np.exp2(rng.uniform(-12, 4, N)).astype(np.float32)
