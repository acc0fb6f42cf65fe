"""NumPy restatement of group-wise weight scales (QModel.group_size): the specification.

A weight W[K, N] has one scale per group of g consecutive k and column: S[G, N], G = K / g, with
quant_parameters' symmetric rule on the group's range clamped to include 0, and the integers of
quantize with S[k // g, n] in the scalar's place.  The product with an int8 activation a (scale
s_a, scalar zero point zpa or none) is, with sg = f32(f32(s_a) * S):
    P_j = sum_{k in group j} (a[m, k] - zpa) b[k, n]                 exact
    acc = 0.0 (f64); acc = acc + f64(sg[j, n]) * f64(P_j) for j = 0 .. G - 1; out = f32(acc)
Nothing here imports numpy_quant.
"""
import numpy as np

from oracle import nq_oracle as O

SHAPES = [(1, 16, 32, 32), (33, 48, 96, 32), (197, 144, 128, 64), (130, 272, 384, 128), (64, 128, 256, 256)]
ZPS = [None, -128, 5, 127]


def group_products(a, b, zpa, g):
    """[G, ..., M, N] float64: the exact integers P_j (every partial sum is an integer below 2^53)."""
    ac = a.astype(np.float64) - (0 if zpa is None else int(zpa))
    bf = b.astype(np.float64)
    return np.stack([ac[..., j * g:(j + 1) * g] @ bf[j * g:(j + 1) * g] for j in range(b.shape[0] // g)])


def group_matmul(a, b, sg, zpa, g):
    """float32 [..., M, N] of integer a [..., M, K], b [K, N] and float32 sg [K / g, N]."""
    assert sg.dtype == np.float32 and sg.shape == (b.shape[0] // g, b.shape[1])
    P = group_products(a, b, zpa, g)
    acc = np.zeros(P.shape[1:], np.float64)
    for j in range(P.shape[0]):
        acc = acc + sg[j].astype(np.float64) * P[j]
    return acc.astype(np.float32)


def group_scales(w, g, bit_width):
    """float32 [K / g, N] of a float32 weight [K, N]."""
    wg = w.reshape(w.shape[0] // g, g, w.shape[1])
    lo, hi = np.minimum(wg.min(axis=1), np.float32(0)), np.maximum(wg.max(axis=1), np.float32(0))
    return np.array([[O.quant_parameters(lo[j, n], hi[j, n], bit_width, False)[0] for n in range(w.shape[1])]
                     for j in range(lo.shape[0])], dtype=np.float32)


def quantize_group(w, S, g, bit_width):
    """int64 [K, N]: quantize without a zero point, element [k, n] with S[k // g, n]."""
    lo, hi = O.qrange(bit_width)
    with np.errstate(all="ignore"):
        t = np.true_divide(w, np.repeat(S, g, axis=0))
        assert t.dtype == np.float32
        return np.rint(np.minimum(np.maximum(t, np.float32(lo)), np.float32(hi))).astype(np.int64)


def saturated(rng, shape):
    """int8, all -128 with about 1 / 16 of the entries redrawn from [-128, -100): products near the
    largest magnitude whose low bits vary."""
    x = np.full(shape, -128, np.int8)
    redraw = rng.random(shape) < 1 / 16
    x[redraw] = rng.integers(-128, -100, size=int(redraw.sum()), dtype=np.int8)
    return x


def near_limit_operands(M, N, g, seed=0):
    """(a, b, sg) with K = 2 g for zpa = 127: saturated a and b, the second group of b with its sign
    flipped (clipped to 127), so |P_j| stays just below 255 * 128 * g with P_0 > 0 > P_1, and at
    g = 16384 nearly no P_j has a float32 image.  sg as in `operands`."""
    rng = np.random.default_rng(7000 + 1000 * M + N + g + seed)
    a, b = saturated(rng, (M, 2 * g)), saturated(rng, (2 * g, N))
    b[g:] = np.clip(-b[g:].astype(np.int16), -127, 127).astype(np.int8)
    return a, b, np.exp2(rng.uniform(-20, 4, size=(2, N))).astype(np.float32)


def many_group_operands(M, N, seed=0):
    """`operands` at g = 32, K = 2048 (64 groups), made to depend on the order of the 64 f64 additions
    in the float32 result (a rounding of 2^-53 relative alone would almost never reach it): group 32
    is group 0 negated (b within +-127), so P_32 = -P_0 for every zpa, and both carry the same
    scale near 2^40.  The other groups alternate between scales near 1 and near 2^-10.  In order,
    the terms of groups 1..31 are each rounded to the ulp of 2^40 |P_0|, the large pair cancels
    exactly and groups 33..63 add with no visible rounding; in any other order other terms, or
    partial sums of them, take that coarse rounding."""
    a, b, sg = operands(M, N, 2048, 32, seed)
    b = np.clip(b, -127, 127)
    a[:, 1024:1056], b[1024:1056] = a[:, :32], -b[:32]
    sg = np.exp2(np.log2(sg) / 12)  # 2^-1.67 .. 2^0.33
    sg[1::2] *= np.float32(2.0 ** -10)
    sg[0] *= np.float32(2.0 ** 40)
    sg[32] = sg[0]
    return a, b, sg.astype(np.float32)


def extreme_scale_rows(N, seed=0):
    """float32 [3, N] for K = 96, g = 32 (|P_j| of random operands is near 2^16), the columns cycling
    through five regimes: the three smallest subnormal scales (a subnormal output); 2^-140 in every
    group (an output near the smallest normal);
    2^-140 beside two ordinary scales; 2^113 beside an ordinary and a subnormal one (+-inf or
    nearly); three ordinary scales as in `operands`."""
    rng = np.random.default_rng(seed + N)
    sg = np.exp2(rng.uniform(-20, 4, size=(3, N)))
    sg[:, 0::5] = np.array([2.0 ** -149, 2.0 ** -147, 2.0 ** -148])[:, None]
    sg[:, 1::5] = 2.0 ** -140
    sg[0, 2::5] = 2.0 ** -140
    sg[0, 3::5], sg[2, 3::5] = 2.0 ** 113, 2.0 ** -140
    return sg.astype(np.float32)


def operands(M, N, K, g, seed=0):
    """int8 a [M, K] and b [K, N] over the full range and sg float32 [K / g, N] log-uniform over
    2^-20..2^4, so that the f64 additions really round."""
    rng = np.random.default_rng(1000 * M + N + K + g + seed)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    b = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    return a, b, np.exp2(rng.uniform(-20, 4, size=(K // g, N))).astype(np.float32)
