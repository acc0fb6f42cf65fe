"""An independent NumPy statement of nqk_compare_stats (numpy_quant/compare.py, nqk_compare.hip),
written without importing that module: the state after one call and after several calls, with
the sums taken lane by lane and fold by fold in the kernel's order, and the metrics a report
derives from a state."""
import math

import numpy as np

CHUNK = 4096
LANES = 256
WORDS = 8


def terms(x, y):
    """(ok, |d|, d * d, x * x) as float64 arrays, zero where the pair is skipped"""
    x = np.asarray(x, dtype=np.float32).ravel()
    y = np.asarray(y, dtype=np.float32).ravel()
    assert x.shape == y.shape
    ok = np.isfinite(x) & np.isfinite(y)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = xd - yd
        return ok, np.where(ok, np.abs(d), 0.0), np.where(ok, d * d, 0.0), np.where(ok, xd * xd, 0.0)


def fold(v):
    v = list(v)
    while len(v) > 1:
        v = [np.float64(a) + np.float64(b) for a, b in zip(v[0::2], v[1::2])]
    return v[0]


def _fold_rows(m):
    """fold() of every row of a [rows, LANES] array at once"""
    while m.shape[1] > 1:
        m = m[:, 0::2] + m[:, 1::2]
    return m[:, 0]


def tree_sum(t) -> np.float64:
    """one call's sum of the float64 terms `t` in the kernel's order"""
    n = t.size
    chunks = -(-n // CHUNK)
    p = np.zeros(chunks * CHUNK)
    p[:n] = t
    # element 4096 c + 1024 j + 4 lane + k
    p = p.reshape(chunks, 4, LANES, 4)
    lane = np.zeros((chunks, LANES))
    for j in range(4):
        for k in range(4):
            lane = lane + p[:, j, :, k]
    partial = _fold_rows(lane)
    lane2 = np.zeros(LANES)
    for c in range(chunks):  # lane c % 256 takes chunk c, in increasing order
        lane2[c % LANES] = lane2[c % LANES] + partial[c]
    return fold(lane2)


def state(x, y, start=None) -> np.ndarray:
    """int64 [8] after one call on (x, y), from `start` or a fresh (all-zero) state"""
    s = np.zeros(WORDS, dtype=np.int64) if start is None else np.array(start, dtype=np.int64)
    x = np.asarray(x, dtype=np.float32).ravel()
    if x.size == 0:
        return s
    ok, ad, dd, xx = terms(x, y)
    f = s.view(np.float64)
    s[0] += int(np.count_nonzero(ok))
    s[1] += int(np.count_nonzero(~ok))
    for w, t in zip((2, 3, 4), (ad, dd, xx)):
        f[w] = f[w] + tree_sum(t)
    f[5] = max(f[5], ad.max())
    return s


def state_of_calls(pairs) -> np.ndarray:
    s = None
    for x, y in pairs:
        s = state(x, y, s)
    return s if s is not None else np.zeros(WORDS, dtype=np.int64)


def metrics(s) -> dict:
    """what a report derives from one state, in float64"""
    s = np.asarray(s, dtype=np.int64)
    count, skipped = int(s[0]), int(s[1])
    sa, sd, sx, mx = (float(v) for v in s.view(np.float64)[2:6])
    if sd == 0.0:
        sqnr = math.inf if sx > 0.0 else math.nan
    elif sx == 0.0:
        sqnr = -math.inf
    else:
        sqnr = 10.0 * math.log10(sx / sd)
    nan = math.nan
    return {"count": count, "nonfinite": skipped, "mean_abs": sa / count if count else nan,
            "mse": sd / count if count else nan, "rms_ref": math.sqrt(sx / count) if count else nan,
            "sqnr_db": sqnr, "max_abs": mx}


def dequantize(q, scale, zp) -> np.ndarray:
    """numpy_quantization.py:37-41 for a scalar or no zero point"""
    q = np.asarray(q).astype(np.int64)
    z = np.int64(0 if zp is None else zp)
    with np.errstate(over="ignore"):
        return ((q - z).astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)


# ----------------------------------------------------------------------------- data
SIZES = [0, 1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 17, 256 * 4096 + 1]


def wide(n, seed=0):
    """normal data over nine decades, a quarter exact zeros (as after a ReLU), some -0.0; y is x
    with an error of about 1 %"""
    rng = np.random.default_rng(1000 + seed + n)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 5, n)).astype(np.float32)
    x[rng.random(n) < 0.25] = 0.0
    x[rng.random(n) < 0.02] = -0.0
    y = (x * (1.0 + 0.01 * rng.standard_normal(n))).astype(np.float32)
    return x, y


# seeds for which the kernel's order, np.sum's and the index order give three different sums of
# d * d at that size (about every other seed does at one size; none of the first 40 at all)
NARROW_SEED = {1024: 2, 1025: 2, 4095: 5, 4096: 5, 4097: 2, 2 * 4096 + 17: 34, 256 * 4096 + 1: 2}


def narrow(n, seed=None):
    """Data on which the summation orders round differently.  Terms from float32 pairs of like
    magnitude carry few bits (d has at most 24, d * d at most 48), so short sums of them are
    exact in every order; here y lies two decades below x, d = x - y spans some 35 bits, d * d
    is rounded to 53, and the terms stay within three decades of each other."""
    seed = NARROW_SEED.get(n, 0) if seed is None else seed
    rng = np.random.default_rng(2000 + seed + n)
    sign = np.array([-1.0, 1.0], np.float32)
    x = rng.uniform(1.0, 30.0, n).astype(np.float32) * rng.choice(sign, n)
    y = rng.uniform(0.01, 0.3, n).astype(np.float32) * rng.choice(sign, n)
    return x, y
