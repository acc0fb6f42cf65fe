"""An independent reference for streamed calibration (numpy_quant/calibration.py, nqk_hist.hip),
written without importing that module: the range rule restated with np.sort and the two ranks,
the histogram with np.bincount."""
import numpy as np

SHIFT = 18
BINS = 1 << (32 - SHIFT)


def key(x) -> np.ndarray:
    """uint32 keys in the order of the floats (-0.0 just before +0.0)"""
    b = np.asarray(x, dtype=np.float32).ravel().view(np.uint32).astype(np.uint64)
    return np.where(b >= 0x80000000, 0xFFFFFFFF - b, b + 0x80000000).astype(np.uint32)


def unkey(k: int) -> np.float32:
    k = int(k)
    bits = k - 0x80000000 if k >= 0x80000000 else 0xFFFFFFFF - k
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def state(x, counts=True) -> np.ndarray:
    """int64 [BINS + 2]: counts, smallest key (fresh 0xFFFFFFFF), largest key (fresh 0)"""
    k = key(x)
    s = np.zeros(BINS + 2, dtype=np.int64)
    s[BINS] = 0xFFFFFFFF
    if k.size:
        if counts:
            s[:BINS] = np.bincount(k >> SHIFT, minlength=BINS)
        s[BINS] = k.min()
        s[BINS + 1] = k.max()
    return s


def sort_ranges(x, percentile) -> tuple:
    """(vmin, vmax) of the elements of x clipped at `percentile`, by sorting"""
    x = np.asarray(x, dtype=np.float32).ravel()
    n = x.size
    assert n > 0
    if np.isnan(x).any():
        return np.float32(np.nan), np.float32(np.nan)
    sk = np.sort(key(x))
    tail = int(n * (100.0 - percentile) / 100.0)
    ku, kl = int(sk[n - 1 - tail]), int(sk[tail])
    bu, bl = ku >> SHIFT, kl >> SHIFT
    vmax = unkey(sk[-1]) if bu == int(sk[-1]) >> SHIFT else unkey((bu << SHIFT) | ((1 << SHIFT) - 1))
    vmin = unkey(sk[0]) if bl == int(sk[0]) >> SHIFT else unkey(bl << SHIFT)
    return vmin, vmax


def bits(v) -> int:
    return int(np.asarray(v, dtype=np.float32).reshape(()).view(np.uint32))


LADDER = np.array([-np.inf, -3.4028235e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.17549435e-38, 1.0, 3.4028235e38, np.inf],
                  dtype=np.float32)
