"""NumPy restatement of the OCP Microscaling formats as this project uses them (QModel.mx_format):
the specification of nqk_quantize_mx and nqk_gemm_mx.

A block is 32 consecutive k of one row.  On finite float32 input:
    amax = max |v|;  e = clip(floor(log2 amax) - emax_elem, -127, 127), from amax's exponent field
    (a subnormal amax gives -127);  scale byte = e + 127 (E8M0), X = 2^e;  an all-zero block: byte 127
    element = round_to_format(v / X): nearest, ties to even, subnormals honoured, saturating at the
    largest finite value; the sign bit of v is kept, also on a zero.
"mxfp8": E4M3, bias 7, largest value 448 (code 0x7e), emax_elem 8, one byte per element.
"mxfp4": E2M1, magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}, emax_elem 2, two elements per byte, even k in
the low nibble.  Nothing here imports numpy_quant.
"""
import numpy as np

EMAX = {"mxfp8": 8, "mxfp4": 2}
MBITS = {"mxfp8": 3, "mxfp4": 1}
BIAS = {"mxfp8": 7, "mxfp4": 1}
TOP = {"mxfp8": 0x7e, "mxfp4": 7}  # the code of the largest finite magnitude


def grid(fmt):
    """float64 magnitudes of the codes 0 .. TOP, ascending."""
    m, bias = MBITS[fmt], BIAS[fmt]
    c = np.arange(TOP[fmt] + 1)
    ex, man = c >> m, c & ((1 << m) - 1)
    return np.where(ex == 0, man * 2.0 ** (1 - bias - m), (1 + man * 2.0 ** -m) * 2.0 ** (ex - bias))


def round_to_format(t, fmt):
    """Codes (sign in the top bit of the format's width) of float64 t, |t| < 2^(emax_elem + 1)."""
    g = grid(fmt)
    a = np.abs(t)
    hi = np.clip(np.searchsorted(g, a, side="left"), 1, len(g) - 1)  # g[hi - 1] <= a <= g[hi] below the top
    lo = hi - 1
    dl, dh = a - g[lo], g[hi] - a  # exact: a and the grid are short binary fractions
    code = np.where((dh < dl) | ((dh == dl) & (hi % 2 == 0)), hi, lo)  # ties to the even code
    code = np.where(a >= g[-1], len(g) - 1, code)
    return (code | (np.signbit(t).astype(np.int64) << (MBITS[fmt] + (4 if fmt == "mxfp8" else 2)))).astype(np.uint8)


def mx_quantize(x, fmt):
    """(codes uint8 [rows, K], one per element, scale bytes uint8 [rows, K / 32]) of float32 x [rows, K]."""
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] % 32 == 0
    b = x.reshape(x.shape[0], -1, 32)
    amax = np.abs(b).max(axis=2)
    field = (amax.view(np.uint32) >> 23).astype(np.int64)  # 0 for a subnormal amax
    e = np.where(amax == 0, 0, np.clip(field - 127 - EMAX[fmt], -127, 127))
    t = b.astype(np.float64) * np.exp2(-e.astype(np.float64))[:, :, None]
    return round_to_format(t, fmt).reshape(x.shape), (e + 127).astype(np.uint8)


def pack(codes, fmt):
    """The stored bytes: codes as they are (mxfp8), or pairs of nibbles, even k low (mxfp4)."""
    return codes if fmt == "mxfp8" else (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack(stored, fmt):
    if fmt == "mxfp8":
        return stored
    out = np.empty((stored.shape[0], 2 * stored.shape[1]), np.uint8)
    out[:, 0::2], out[:, 1::2] = stored & 15, stored >> 4
    return out


def mx_dequantize(codes, scales, fmt):
    """float64 [rows, K], exact."""
    sbit = 0x80 if fmt == "mxfp8" else 8
    mag = grid(fmt)[(codes & (sbit - 1)).astype(np.int64)]
    val = np.where(codes & sbit, -mag, mag)
    return val * np.repeat(np.exp2(scales.astype(np.float64) - 127), 32, axis=1)


def mx_matmul_ref(a, a_scales, a_fmt, bt, b_scales, b_fmt):
    """(sum_k f64(a) f64(b), sum_k |a b|) [M, N] float64 of codes a [M, K] and bt [N, K]."""
    da, db = mx_dequantize(a, a_scales, a_fmt), mx_dequantize(bt, b_scales, b_fmt)
    return da @ db.T, np.abs(da) @ np.abs(db).T


def planted_blocks(fmt):
    """float32 [11, 160]: rows of five blocks that cover every midpoint between adjacent code points at
    both signs (amax = 2^emax, so X = 1), an amax that is a power of two, amax / X in the saturating
    gap, an all-zero block, float32 subnormals, a block whose only large value is negative, one value
    2^30 times the rest, magnitudes near 2^100, an amax in the smallest normal binade (e clipped at
    -127), and negative zeros."""
    g = grid(fmt)
    mid = (g[:-1] + g[1:]) / 2
    top = 2.0 ** EMAX[fmt]
    rng = np.random.default_rng(len(g))
    x = rng.standard_normal((11, 160)).astype(np.float32)
    m = np.resize(mid, 155)
    x[0, :155], x[1, :155] = m, -m
    x[0, 155:], x[1, 155:] = top, -top  # every block of rows 0 and 1 has amax = 2^emax exactly
    x[0:2] = x[0:2].reshape(2, 32, 5).transpose(0, 2, 1).reshape(2, 160)  # column 155 + j lands in block j
    x[2] = rng.uniform(-1, 1, 160) * 2.0 ** -3
    x[2, ::32] = 2.0 ** -3  # amax a power of two
    x[3] = rng.uniform(-1, 1, 160)
    x[3, 5::32] = np.float32(1.99)  # 1.99 * 2^emax lies above the largest finite value: saturates
    x[3, 6::32] = np.float32(-1.97)
    x[4, 32:64] = 0  # an all-zero block between ordinary ones
    x[5] = (rng.integers(-2 ** 22, 2 ** 22, 160) * 2.0 ** -149).astype(np.float32)  # subnormals: e = -127
    x[6] = rng.uniform(0, 1, 160)
    x[6, 7::32] = -37.5  # the block's amax is negative
    x[7] = rng.standard_normal(160) * 2.0 ** -30
    x[7, 9::32] = 1.25
    x[8] = rng.standard_normal(160) * 2.0 ** 100
    x[9] = rng.uniform(-1, 1, 160) * 2.0 ** -126
    x[9, 3::32] = 1.5 * 2.0 ** -126  # the smallest normal binade: e is clipped at -127, amax / X = 3
    x[10] = -0.0
    return x


def scaled_normal(rows, cols, seed):
    """float32 [rows, cols]: normal data times a per-block 2^U[-20, 20]."""
    rng = np.random.default_rng(seed + 100 * rows + cols)
    s = np.exp2(rng.integers(-20, 21, (rows, cols // 32)).astype(np.float64))
    return (rng.standard_normal((rows, cols)) * np.repeat(s, 32, axis=1)).astype(np.float32)


def exact_fixture(M, N, K, a_fmt, b_fmt, seed=0):
    """Codes and scale bytes (a, a_scales, bt, b_scales) of integer elements in [-4, 4] with an exponent
    in [-2, 2] per (row, block) and (column, block), neighbours differing along both axes."""
    rng = np.random.default_rng(seed + 1000 * M + 10 * N + K)

    def side(rows, fmt, shift):
        v = rng.integers(-4, 5, (rows, K)).astype(np.float64)
        r, b = np.indices((rows, K // 32))
        exps = (r + 2 * b + shift + rng.integers(0, 2, 1)) % 5 - 2  # differs from both neighbours
        return round_to_format(v, fmt), (exps + 127).astype(np.uint8)  # integers up to 4 lie on both grids

    return side(M, a_fmt, 0) + side(N, b_fmt, 1)
