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


def operands(M, N, K, g, seed=0):
    """int8 a [M, K] and b [K, N] over the full range and sg float32 [K / g, N] log-uniform over
    2^-20..2^4, so that the f64 additions really round."""
    rng = np.random.default_rng(1000 * M + N + K + g + seed)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    b = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    return a, b, np.exp2(rng.uniform(-20, 4, size=(K // g, N))).astype(np.float32)
