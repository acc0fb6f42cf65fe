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


def extreme_positions(cols, long_path=False, big=1000.0, seed=0):
    """(x float32 [2 P, cols], positions): rows of noise within +-1; row i holds +big and row P + i
    holds -big at positions[i]: the first and last columns, the edges of a lane's first chunk and
    of the first 256-column block, and the first column of every block; for the two-pass kernel
    also 1023 and 1024, where the share of another wave and the next loop trip begin."""
    pos = {0, 3, 4, 255, 256, cols - 1} | set(range(0, cols, 256))
    if long_path:
        pos |= {1023, 1024}
    pos = sorted(p for p in pos if 0 <= p < cols)
    rng = np.random.default_rng(seed + cols)
    x = rng.uniform(-1, 1, (2 * len(pos), cols)).astype(np.float32)
    for i, p in enumerate(pos):
        x[i, p], x[len(pos) + i, p] = big, -big
    return x, pos


def range_extremes(cols=70):
    """float32 [6, cols], zeros past the listed values: a range hi - lo that overflows float32
    (s = inf, z = qlo, every q = qlo); FLT_MAX in a positive row; a subnormal scale; a range that
    underflows to s = 0 at 8 bits but not at 4; the smallest normal magnitudes; -0.0 among +0.0."""
    fmax = np.finfo(np.float32).max
    rows = [[3e38, -3e38, 1, 0, -1],
            [fmax, 1e38, 1, 1e-38, 3e38],
            [2.0 ** -140, 0, 2.0 ** -145, -2.0 ** -149, 2.0 ** -141],
            [1e-44, -1e-44, 0, 1e-45, 0],
            [1.2e-38, -1.2e-38, 0, 1.2e-38, -1.2e-38],
            [-0.0, 0.0, -0.0, 0.0, -0.0]]
    x = np.zeros((len(rows), cols), np.float32)
    for i, r in enumerate(rows):
        x[i, :len(r)] = np.array(r, np.float32)
    x[5, 5::2] = -0.0
    return x


def near_limit_operands(M, N, K, seed=0):
    """(a, w, z, s, sw) with |P - z colsum| just below 255 * 128 * K: a and w all -128 with about
    1 / 16 of the entries redrawn from [-128, -100), the right half of w's columns negated (clipped
    to 127), z = 127; the last row of a is negated the same way and has z = -128.  At K = 65520
    the values span nearly all of int32 and nearly none has a float32 image.  s, sw as in
    gemm_operands."""
    rng = np.random.default_rng(seed + 7000 + 1000 * M + 10 * N + K)

    def saturated(shape):
        x = np.full(shape, -128, np.int8)
        redraw = rng.random(shape) < 1 / 16
        x[redraw] = rng.integers(-128, -100, size=int(redraw.sum()), dtype=np.int8)
        return x

    a, w = saturated((M, K)), saturated((K, N))
    w[:, N // 2:] = np.clip(-w[:, N // 2:].astype(np.int16), -127, 127).astype(np.int8)
    a[-1] = np.clip(-a[-1].astype(np.int16), -127, 127).astype(np.int8)
    z = np.full(M, 127, np.int64)
    z[-1] = -128
    s = np.exp2(rng.uniform(-12, 4, M)).astype(np.float32)
    return a, w, z, s, np.exp2(rng.uniform(-12, 4, N)).astype(np.float32)


def integers(a, w, z):
    """(P, P - z colsum) int64 [M, N]: the integers nqk_qgemm_rows holds in int32 (through float64,
    exact below 2^53)."""
    P = np.matmul(a.astype(np.float64), w.astype(np.float64)).astype(np.int64)
    return P, P - z.astype(np.int64)[:, None] * w.astype(np.int64).sum(axis=0)[None, :]


def extreme_scales(M, N, seed=0):
    """(s [M], sw [N]) of gemm_operands' range, with rows and columns exchanged for powers of two
    whose float32 products s[m] * sw[n] are zero (2^-100 * 2^-60), subnormal (2^-100 * 2^-40),
    ordinary, or 2^127 (2^100 * 2^27: inf against an integer of 2 or more); no product is inf, so
    no output is 0 * inf."""
    rng = np.random.default_rng(seed + M + N)
    s, sw = np.exp2(rng.uniform(-12, 4, M)), np.exp2(rng.uniform(-12, 4, N))
    s[0::5], s[1::5], s[2::5] = 2.0 ** -100, 2.0 ** 100, 2.0 ** -126
    sw[0::6], sw[1::6], sw[2::6] = 2.0 ** -40, 2.0 ** 27, 2.0 ** -60
    return s.astype(np.float32), sw.astype(np.float32)


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
