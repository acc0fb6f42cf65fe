"""Inputs of tests/test_gpu_l1_kernels.py and their NumPy references: the per-node integer path
(nqk_quantize, nqk_dequantize, nqk_requantize, nqk_rowsum, nqk_relu_q, nqk_qgemm_i8 and
nqk_qgemm_generic) at the edges where such kernels go wrong.  Built on the host alone, no device
import, so that tests/test_l1_cases_ref.py can assert without a GPU that every table reaches the
edge it claims.  References are oracle.nq_oracle.quantize / dequantize / q_matmul / requantize
(pinned to the reference's fixtures by tests/test_oracle.py), np.where(q < zp, zp, q) for relu and
a.sum(-1) for row sums; integers are int64 throughout.  Every builder is seeded by its own
arguments and cached: one reference per case, shared by all tests, never modified."""
import functools
import zlib

import numpy as np

from oracle import nq_oracle as O

F32 = np.float32
I64 = np.int64
INT64_MIN = np.iinfo(np.int64).min


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def zp_arr(zp):
    """A zero point as the reference passes it: None or a 0-d int64 array."""
    return None if zp is None else np.array(zp, I64)


def storage(bit_width):
    """The narrow storage the device keeps for a bit width (kernels.storage_dtype)."""
    return np.dtype(np.int8 if bit_width <= 8 else np.int16 if bit_width <= 16 else
                    np.int32 if bit_width <= 32 else np.int64)


# ----------------------------------------------------------------------------- group 1: quantize
BIT_WIDTHS = (1, 2, 4, 8, 12, 16, 26, 32)
QPARAMS = ((1, None), (0.5, None), (0.0213, None), (1, 0), (0.5, 3), (0.0213, 17), (0.05, -140), (1, -138),
           (0.031, 1 << 20))
POW2_SCALES = (1, 0.5)  # x / s is exact: (k + 0.5) * s quantizes from an exact tie
TIE_K = np.arange(-300, 300)
LADDER = np.arange(-1, 1.25, 0.25)
REL = np.array([-2.0 ** -10, -2.0 ** -20, 2.0 ** -20, 2.0 ** -10])  # steps a float32 near 2^31 can take
FLT_MAX = np.finfo(F32).max
SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], F32)


def quant_parts(bw, scale, zp):
    """The pieces of the quantize input for (bw, scale, zp), float32 each:
    normals  seeded normals * 3;
    ties     (k + 0.5 - z) * s for k in -300..299 and z in {0, zp}: exact ties of the quotient (and of
             zp + quotient) when s is a power of two, near-ties of a rounded division otherwise;
    ladder   (bound - z + d) * s for both clip bounds, d in -1..1 in steps of 0.25, and
             (bound - z) * (1 + r) * s for the relative steps REL (at 26 and 32 bits float32 cannot
             take steps of 0.25 around the bound);
    special  +-0, +-1e-30, +-1e30, +-FLT_MAX, +-inf, NaN."""
    s = float(F32(scale))
    lo, hi = O.qrange(bw)
    zs = (0,) if not zp else (0, zp)
    normals = (_rng("quant", bw, scale).standard_normal(600) * 3).astype(F32)
    ties = np.concatenate([(TIE_K + 0.5 - z) * s for z in zs]).astype(F32)
    lad = []
    for z in zs:
        for b in (lo, hi):
            lad += [(b - z + LADDER) * s, (b - z) * (1 + REL) * s]
    ladder = np.concatenate(lad).astype(F32)
    return normals, ties, ladder, SPECIALS


@functools.lru_cache(maxsize=None)
def quant_input(bw, scale, zp):
    with np.errstate(over="ignore"):
        return _frozen(np.concatenate(quant_parts(bw, scale, zp)))


def preclip(x, scale, zp):
    """The value the reference clips and rounds (numpy_quantization.py:26-29): f32(x / s), plus
    f64(zp) in float64 when there is a zero point."""
    with np.errstate(all="ignore"):
        t = np.true_divide(np.asarray(x, F32), F32(scale))
        return t if zp is None else np.float64(zp) + t.astype(np.float64)


def quantize_ref(x, bw, scale, zp):
    """O.quantize with NaN pinned to INT64_MIN, the x86 float -> int64 conversion the kernels
    document (nqk_quant.hip); test_l1_cases_ref.py asserts that this host's NumPy gives the same."""
    with np.errstate(all="ignore"):
        q = O.quantize(np.asarray(x, F32), bw, F32(scale), zp_arr(zp))
    return _frozen(np.where(np.isnan(x), INT64_MIN, q))


@functools.lru_cache(maxsize=None)
def quant_ref(bw, scale, zp):
    return quantize_ref(quant_input(bw, scale, zp), bw, scale, zp)


def half_away(u):
    """Round half away from zero, the variant a wrong kernel would most likely use."""
    return np.sign(u) * np.floor(np.abs(u) + 0.5)


# flat kernel: lengths around the 4-element vector body and one past the grid (4096 * 256 * 4)
FLAT_N = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 4 * 2 ** 20 + 7)
FLAT_GRID = 4096 * 256 * 4
FLAT_QP = (8, 0.5, 3)      # multiples of 0.25 over a scale of 0.5: half the quotients are ties
UNALIGNED_N = 1027


@functools.lru_cache(maxsize=None)
def flat_input(n):
    x = np.rint(_rng("flat", n).standard_normal(n) * 160) / 4
    return _frozen(x.astype(F32))


# row kernel: (rows, len); the last has more rows than 4096 blocks * 4 waves
ROW_SHAPES = ((1, 1), (3, 63), (5, 64), (7, 65), (2, 4099), (300, 197), (16384 + 3, 5))
ROW_GRID = 4096 * 4
ROW_QP = ((8, 0.5, None), (8, 0.5, 3), (12, 0.03125, None), (12, 0.03125, -140))


@functools.lru_cache(maxsize=None)
def row_input(rows, length):
    x = np.rint(_rng("rows", rows, length).standard_normal((rows, length)) * 160) / 4
    return _frozen(x.astype(F32))


# ----------------------------------------------------------------------------- group 2: de/requantize
BIG_SHAPE = (8, 12)
BIG_SCALE = F32(0.0047)
BIG_RES_SCALE = F32(0.37)
ZP_FORMS = ("none", "scalar", "row", "col", "full")


@functools.lru_cache(maxsize=None)
def big_acc():
    """Accumulators around +-2^24, +-2^31, +-2^53, +-2^54 and +-2^62 with offsets -3..3 and
    +-(2^9 + 1), and the three named ones: 2^53 + 1 and 2^53 + 3 are exact half-way cases of the
    int64 -> float64 conversion (they round to even: 2^53 and 2^53 + 4), -2^62 - 2^9 - 1 lies just
    past half-way (spacing 2^10) and rounds away."""
    vals = [2 ** 53 + 1, 2 ** 53 + 3, -2 ** 62 - 2 ** 9 - 1]
    for e in (24, 31, 53, 54, 62):
        for sign in (1, -1):
            for off in (-3, -2, -1, 0, 1, 2, 3, 2 ** 9 + 1, -2 ** 9 - 1):
                vals.append(sign * 2 ** e + off)
    vals += [0, 1, -1]
    assert len(vals) == BIG_SHAPE[0] * BIG_SHAPE[1]
    return _frozen(np.array(vals, I64).reshape(BIG_SHAPE))


@functools.lru_cache(maxsize=None)
def zp_form(form, shape):
    """A zero point of one broadcast form against `shape` (None, 0-d, (R, 1), (1, C), (R, C))."""
    rng = _rng("zpform", form, shape)
    r, c = shape
    if form == "none":
        return None
    if form == "scalar":
        return np.array(-37, I64)
    return _frozen(rng.integers(-100, 101, {"row": (r, 1), "col": (1, c), "full": (r, c)}[form]).astype(I64))


def centred(acc, zp):
    return acc if zp is None else acc - zp


def f64_inexact(v):
    """Which int64 values float64 cannot hold, and which of those lie exactly half-way."""
    v = np.asarray(v, I64).reshape(-1)
    py = [int(t) for t in v]
    f = [int(float(t)) for t in py]
    inexact = np.array([a != b for a, b in zip(py, f)])
    half = []
    for t in py:
        m = abs(t)
        ulp = 1 << max(0, m.bit_length() - 53)
        half.append(ulp > 1 and m % ulp == ulp // 2)
    return inexact, np.array(half)


TIE_BW = (2, 4, 8, 16, 32)
TIE_RES_ZP = (None, -3, 200)
TIE_ARR_SCALE = F32(0.5)
TIE_RES_SCALE = F32(1)


@functools.lru_cache(maxsize=None)
def tie_acc(bw):
    """Odd accumulators (acc * 0.5 is exactly k + 0.5) in -601..601, then accumulators two apart and
    their odd neighbours around both clip bounds of `bw` as each result zero point z of TIE_RES_ZP
    places them (2 * (bound - z + j) + {0, 1}, j in -3..3)."""
    lo, hi = (int(v) for v in O.qrange(bw))
    odd = np.arange(-601, 602, 2)
    edge = [2 * (b - (z or 0) + j) + o for z in TIE_RES_ZP for b in (lo, hi) for j in range(-3, 4) for o in (0, 1)]
    edge += [int(2 * (b - (z or 0)) * (1 + r)) for z in TIE_RES_ZP for b in (lo, hi) for r in REL]  # float32 steps
    return _frozen(np.concatenate([odd, np.array(edge, I64)]).astype(I64))


STRIDE_SHAPE = (1049, 1001)  # more elements than 4096 blocks * 256 threads
STRIDE_GRID = 4096 * 256


@functools.lru_cache(maxsize=None)
def stride_acc():
    rng = _rng("stride")
    acc = rng.integers(-2 ** 20, 2 ** 20, STRIDE_SHAPE).astype(I64)
    zp = rng.integers(-2 ** 12, 2 ** 12, (1, STRIDE_SHAPE[1])).astype(I64)
    return _frozen(acc), _frozen(zp)


# bit width 32 without a result zero point: results that reach the float32 bound 2^31
def sat32_acc():
    """acc * 0.5 / 1 around +-2^31: float32 rounds 2^31 - 1 up to 2^31, which the reference keeps."""
    b = 2 ** 32
    return _frozen(np.array([b + 8, b, b - 2, b - 128, b - 512, 2 ** 31, 5, -5, -b + 512, -b, -b - 8, -2 ** 40,
                             2 ** 40], I64))


# ----------------------------------------------------------------------------- group 3: matmul
MM_SHAPES = (
    ("generic", (5, 3), (3, 2), False),
    ("mfma-padded-k", (33, 40), (40, 35), False),
    ("mfma-tile-edge", (129, 64), (64, 130), False),
    ("b-broadcast", (3, 33, 40), (40, 35), False),
    ("b-broadcast-weight", (3, 33, 40), (40, 35), True),
    ("a-broadcast", (33, 40), (4, 40, 35), False),
    ("outer-inner", (2, 1, 33, 40), (1, 3, 40, 35), False),
    ("equal-batches", (2, 3, 33, 40), (2, 3, 40, 35), False),
    ("materialised-generic", (2, 1, 3, 9, 16), (1, 4, 1, 16, 9), False),
    ("materialised-mfma", (2, 1, 3, 33, 40), (1, 4, 1, 40, 35), False),
    ("grid-stride", (1049, 16), (16, 1001), False),
)
MM_NAMES = tuple(s[0] for s in MM_SHAPES)
ZP_PAIRS = ((None, None), (-138, None), (None, 11), (-138, 11))
MM_BW = (8, 4, 12)
MM_SA, MM_SB = F32(0.031), F32(0.0047)
MM_RES_ZP = (None, -3)
BIASES = ("none", "vector", "int8")
MFMA_MIN_WORK = 1 << 15
# (name, bw, zb) -> seed salt, where the default seed misses a condition of test_l1_cases_ref.py (the
# 10 outputs of the generic case lie in two column clusters at 4 bits: few seeds spread them out)
MM_SALT = {("generic", 4, None): 983, ("generic", 4, 11): 1, ("mfma-padded-k", 4, 11): 2}


def mm_shape(name):
    return MM_SHAPES[MM_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def mm_operands(name, bw, zb):
    """A uniform over -hi..hi (mean zero); B normal around its zero point when that lies in the range
    of `bw`, else around 0; both with the range's two extremes planted.  With A of mean zero or
    B - zb of mean zero the products (a - za)(b - zb) spread to both sides of zero, which the
    two-sided clip condition of the requantize cases needs."""
    _, sa, sb, _ = mm_shape(name)
    rng = _rng("mm", sa, sb, bw, zb, MM_SALT.get((name, bw, zb), 0))
    lo, hi = (int(v) for v in O.qrange(bw))
    centre = zb if zb is not None and lo <= zb <= hi else 0
    a = rng.integers(-hi, hi + 1, sa).astype(I64)
    b = np.clip(np.rint(centre + rng.standard_normal(sb) * (hi - lo) / 5), lo, hi).astype(I64)
    a.reshape(-1)[:2] = (lo, hi)
    b.reshape(-1)[:2] = (hi, lo)
    return _frozen(a), _frozen(b)


def zp_term(a, b, za, zb, roll_row=None, roll_col=None):
    """The zero-point term of O.q_matmul, optionally with A's row sums (`roll_row`) or B's column
    sums (`roll_col`) rolled by one along that batch axis: what a kernel that indexed the wrong
    batch would subtract."""
    if za is None and zb is None:
        return None
    row = a.sum(axis=-1, keepdims=True)
    col = b.sum(axis=-2, keepdims=True)
    if roll_row is not None:
        row = np.roll(row, 1, axis=roll_row)
    if roll_col is not None:
        col = np.roll(col, 1, axis=roll_col)
    k = a.shape[-1]
    if za is None:
        return row * zb
    if zb is None:
        return col * za
    return row * zb + col * za - za * zb * k


def clip_fractions(q, bw):
    lo, hi = (int(v) for v in O.qrange(bw))
    return float(np.mean(q == lo)), float(np.mean(q == hi)), float(np.mean((q > lo) & (q < hi)))


def _pick_res_scale(acc, s, term, rz, bw, one_sided):
    """The result scale that puts the lowest tenth of the dequantized reference on the lower clip
    bound and the highest tenth on the upper one, whichever of the two asks for the smaller scale
    (above 2^17 outputs: 10.5 % of a sample): an output is `lo` from rz + d / rs <= lo + 0.5 down
    and `hi` from hi - 0.5 up.  test_l1_cases_ref.py asserts on every output that a tenth sit on each bound
    and half inside.  A product of one sign (`one_sided`) reaches one bound only, and is held to
    that one."""
    flat = acc.reshape(-1)
    idx = np.arange(0, flat.size, max(1, flat.size // (1 << 17)))
    tsub = None if term is None else np.broadcast_to(term, acc.shape).reshape(-1)[idx]
    d = O.dequantize(flat[idx], s, tsub).astype(np.float64)
    lo, hi = O.qrange(bw)
    d.sort()
    k = int(np.ceil((0.1 if d.size == flat.size else 0.105) * d.size))
    q_lo, q_hi = d[k - 1], d[d.size - k]
    cands = []
    if q_lo < 0:
        cands.append(q_lo / (lo + 0.5 - (rz or 0)))
    if q_hi > 0:
        cands.append(q_hi / (hi - 0.5 - (rz or 0)))
    assert cands and (one_sided or len(cands) == 2)
    return F32(min(cands) * (1 - 2.0 ** -20))


@functools.lru_cache(maxsize=None)
def mm_case(name, bw, zpair):
    """Everything the reference says about one product: operands, acc, scale, term, the dequantized
    accumulator, and per bias kind and result zero point the result scale and requantized output."""
    za, zb = zpair
    a, b = mm_operands(name, bw, zb)
    acc, s, term = O.q_matmul(a, MM_SA, zp_arr(za), b, MM_SB, zp_arr(zb))
    term_ref = zp_term(a, b, za, zb)
    assert (term is None) == (term_ref is None) and (term is None or np.array_equal(term, term_ref))
    n = acc.shape[-1]
    rng = _rng("bias", name, bw, zpair, MM_SALT.get((name, bw, zb), 0))
    d = O.dequantize(acc, s, term)
    lim = 2 ** (4 * bw - 1) - 1
    spread = int(min(lim, max(1.0, float(np.std(centred(acc, term))) / 4)))
    biases = {"none": None,
              "vector": rng.integers(-spread, spread + 1, n).astype(I64),
              "int8": rng.integers(-min(128, spread), min(127, spread) + 1, n).astype(I64)}
    one_sided = bool((d < 0).all() or (d > 0).all())
    out = {}
    for kind, bias in biases.items():
        accb = acc if bias is None else acc + bias
        for rz in MM_RES_ZP:
            rs = _pick_res_scale(accb, s, term, rz, bw, one_sided)
            out[kind, rz] = (rs, _frozen(O.requantize(accb, s, term, rs, zp_arr(rz), bw)))
    return dict(a=a, b=b, za=za, zb=zb, acc=_frozen(acc), s=s, term=term, deq=_frozen(d),
                biases={k: (None if v is None else _frozen(v)) for k, v in biases.items()},
                one_sided=one_sided, requant=out)


# nqk_qgemm_generic with operands of two storages: (dtype of A, its magnitude, dtype of B, its magnitude)
MIXED = ((np.int8, 2 ** 7, np.int64, 2 ** 48), (np.int32, 2 ** 28, np.int16, 2 ** 15),
         (np.int64, 2 ** 28, np.int64, 2 ** 28))
MIXED_SHAPE = ((37, 50), (50, 29))


@functools.lru_cache(maxsize=None)
def mixed_case(i):
    ta, ma, tb, mb = MIXED[i]
    rng = _rng("mixed", i)
    a = rng.integers(-ma, ma, MIXED_SHAPE[0]).astype(ta)
    b = rng.integers(-mb, mb, MIXED_SHAPE[1]).astype(tb)
    a[0, :] = ma - 1   # one output of one sign throughout: the largest sum
    b[:, 0] = mb - 1
    ref = [[sum(int(x) * int(y) for x, y in zip(ra, cb)) for cb in b.T] for ra in a]
    exact = np.array(ref, dtype=object)
    assert max(abs(int(v)) for v in exact.reshape(-1)) < 2 ** 63
    return _frozen(a), _frozen(b), _frozen(exact.astype(I64))


# ----------------------------------------------------------------------------- group 4: accumulator width
# 131056: the last multiple of 16 below the bound 2^17, exact in int32; 131072: one product sum is
# 2^31; 140000 (a multiple of 16) and 140001 (not one, so an int8 route would pad it): both
# same-sign sums pass 2^31
ACC_K = (131056, 131072, 140000, 140001)
ACC_ZP = ((None, None), (-138, 11))


@functools.lru_cache(maxsize=None)
def acc_case(k, zpair):
    """A (2, K): a row of -128 and a row of 127; B (K, 2): a column of -128 and a column of 127.
    K = 131072 puts (-128)^2 * K at exactly 2^31."""
    a = np.repeat(np.array([[-128], [127]], I64), k, axis=1)
    b = np.repeat(np.array([[-128, 127]], I64), k, axis=0)
    acc, s, term = O.q_matmul(a, MM_SA, zp_arr(zpair[0]), b, MM_SB, zp_arr(zpair[1]))
    return _frozen(a), _frozen(b), _frozen(acc), s, term


def wrap32(v):
    return np.asarray(v, I64).astype(np.int32).astype(I64)


# ----------------------------------------------------------------------------- group 5: relu_q, rowsum
RELU_DTYPES = (np.int8, np.int16, np.int32, np.int64)
RELU_N = (1, 255, 2 ** 20 + 5)   # the last is past 4096 blocks * 256 threads


def relu_zero_points(dt):
    """(zero point, whether it lies outside the storage range): inside, at both ends, and (narrow
    storage only) outside on either side."""
    info = np.iinfo(dt)
    zps = [(3, False), (info.min, False), (info.max, False)]
    if np.dtype(dt) != np.int64:
        zps += [(info.min - 5, True), (info.max + 5, True)]
    return zps


@functools.lru_cache(maxsize=None)
def relu_case(dt, n, zp):
    """n values of storage `dt`: zp - 1, zp, zp + 1 and both storage extremes (those that fit, as
    many as n allows), the rest uniform over the whole range; and np.where(q < zp, zp, q)."""
    info = np.iinfo(dt)
    rng = _rng("relu", np.dtype(dt).name, n, zp)
    q = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True)
    named = [v for v in (zp, zp - 1, zp + 1, info.min, info.max) if info.min <= v <= info.max]
    m = min(n, len(named))
    q[:m] = named[:m]
    ref = np.where(q < zp, I64(zp), q)
    return _frozen(q.astype(dt)), _frozen(ref)


# (batch, rows, k, ld, bstride): ld > k pads the rows, bstride > rows * ld pads the matrices; the last
# has batch * rows = 16384 + 3 sums, more than 4096 blocks * 4 waves
ROWSUM_SHAPES = ((1, 1, 1, 1, 1), (2, 3, 63, 63, 189), (2, 3, 64, 70, 250), (3, 5, 65, 80, 407),
                 (1, 4, 200, 200, 800), (2, 2, 200, 203, 411), (2341, 7, 5, 6, 50))


@functools.lru_cache(maxsize=None)
def rowsum_case(dt, shape):
    batch, rows, k, ld, bstride = shape
    assert ld >= k and bstride >= rows * ld
    info = np.iinfo(dt)
    lim = min(info.max, 2 ** 50)
    buf = _rng("rowsum", np.dtype(dt).name, shape).integers(-lim - 1, lim, batch * bstride, dtype=np.int64,
                                                          endpoint=True)
    idx = (np.arange(batch)[:, None, None] * bstride + np.arange(rows)[None, :, None] * ld
           + np.arange(k)[None, None, :])
    assert idx.max() < buf.size
    return _frozen(buf.astype(dt)), _frozen(buf[idx].sum(-1).reshape(-1))
