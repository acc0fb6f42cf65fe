"""Inputs of tests/test_gpu_ln_reference.py (nqk_ln_quant on every kernel form) and of the
residual-row cases of the fused LayerNorm epilogue (tests/_fused_cases.py), with their references:
the oracle's LayerNormalization (oracle/nq_oracle.py::_float_op) followed by O.quantize, and nothing
else.  Built on the host from NumPy alone, cached, one reference per case, never modified; the
conditions that make a case worth running are asserted on the reference by
tests/test_ln_cases_ref.py without a GPU.

Why these inputs: the int8 bytes of benign rows (a few units of standard deviation around a small
mean) do not see the last bits of the mean, the variance or 1 / sqrt, so a kernel that sums in
another order, takes a faster reciprocal square root or fuses the last multiply-add passes on them.
The kinds:

a  ill-conditioned rows, x = c + sigma * randn with |c| / sigma up to 4 10^5: the mean's rounding
   error is a visible fraction of sigma, so the order of the mean's sum shows in the bytes;
b  rows of +-(1 + 1e-4 u) with gamma ~ 0.75, beta ~ 0.25, s = 2^-20, zp = -2^20: the positive half
   of a row has y within 1.1e-4 of 1, where one ulp of y is 1/8 or 1/16 of an output step, so the
   variance's tree, the square root and division, contraction and the grouping of the last step
   show; the negative half clips low ("bm": mirrored through gamma ~ -0.75);
c  rows of +-2^j with balanced signs: mean 0, variance 4^j, everything exact, gamma and beta
   multiples of 1/16 (half the betas 1/32 more), s = 2^-4: half the elements are exact rounding ties;
d  random rows at the parameter edges: bit widths 1 - 4 and 8, zero points up to +-(2^20 + 1),
   scales 2^-101 and 2^101;
e  degenerate rows: constants, zeros, -0.0, magnitudes 1e18 and 1e-18 around a row of zeros;
f  an inf row and NaN rows among finite rows (out of contract: only the finite rows are compared).

ln_restated() states the chain step by step in NumPy and, on request, with one deliberate mistake;
the host test uses it to show that a case can see that mistake."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import nq_oracle as O

LnCase = namedtuple("LnCase", "kind cols rows eps var", defaults=(67, 1e-12, 0))
EPS = (1e-12, 1e-5)            # the ViT graphs' epsilon and the ONNX default
A_PARAMS = ((4096.0, 0.01), (-3000.0, 0.02), (64.0, 0.01))   # (c, sigma), row r takes entry r % 3
C_ZP = (3, -4, -(1 << 20), (1 << 20) + 1)                    # odd, even, the magic-number limit, one beyond (f64)
P20 = 1 << 20
# (bit width, zero point, scale): scales a few units of standard deviation across the range
_S = {8: 0.031, 4: 0.45, 3: 0.8, 2: 2.0, 1: 2.0}
D_PARAMS = ([(bw, zp, _S[bw]) for bw, zp in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, -2), (4, 0), (4, 5), (8, 0), (8, 140),
                                              (8, -300), (8, P20), (8, -P20), (8, P20 + 1), (8, -P20 - 1), (2, P20),
                                              (3, -P20 - 1))]
            + [(8, 3, 2.0 ** -101), (8, 3, 2.0 ** 101)])
MISTAKES = ("mean_seq", "var_seq", "inv_ulp", "inv_f64", "fma", "regroup")


def reference(x, gamma, beta, eps, scale, zp, bw):
    y = O._float_op("LayerNormalization", [O.F(x), O.F(gamma), O.F(beta)], {"axis": -1, "epsilon": eps})[0][1]
    assert y.dtype == np.float32
    return O.quantize(y, bw, np.float32(scale), np.int64(zp))


def _seq_sum(v):
    return np.cumsum(v, axis=-1, dtype=np.float32)[..., -1:]


def ln_restated(x, gamma, beta, eps, scale, zp, bw, mistake=None):
    """The reference chain one f32 operation at a time; mistake=None gives the reference's bytes
    (asserted by the host test), otherwise one of MISTAKES is made:
    mean_seq / var_seq  the sum of the mean / of the variance left to right in f32;
    inv_ulp             1 / sqrt one ulp up;
    inv_f64             f32(1 / sqrt(f64(var + eps)));
    fma                 the last step as one rounding of the f64 p g + b, p the f32 product d inv;
    regroup             d (inv g) + b."""
    assert mistake is None or mistake in MISTAKES
    n = np.float32(x.shape[-1])
    with np.errstate(all="ignore"):
        mean = (_seq_sum(x) if mistake == "mean_seq" else x.sum(axis=-1, keepdims=True)) / n
        d = x + (-mean)
        sq = d * d
        var = (_seq_sum(sq) if mistake == "var_seq" else sq.sum(axis=-1, keepdims=True)) / n
        ve = var + np.float32(eps)
        if mistake == "inv_f64":
            inv = (1.0 / np.sqrt(ve.astype(np.float64))).astype(np.float32)
        else:
            inv = np.float32(1) / np.sqrt(ve)
        if mistake == "inv_ulp":
            inv = np.nextafter(inv, np.float32(np.inf))
        if mistake == "fma":
            y = ((d * inv).astype(np.float64) * gamma.astype(np.float64) + beta.astype(np.float64)).astype(np.float32)
        elif mistake == "regroup":
            y = d * (inv * gamma) + beta
        else:
            y = (d * inv) * gamma + beta
    assert y.dtype == np.float32
    return O.quantize(y, bw, np.float32(scale), np.int64(zp))


def rows_changed(d, mistake, first=64):
    """Of the first `first` rows of case d, how many have a byte changed by `mistake`."""
    sl = slice(0, first)
    q = ln_restated(d["x"][sl], d["gamma"], d["beta"], d["eps"], d["scale"], d["zp"], d["bw"], mistake)
    return int((q != d["ref"][sl]).any(axis=-1).sum())


def _signs(rng, rows, cols):
    """+-1 per element, each row a random permutation of cols / 2 of either sign."""
    base = np.where(np.arange(cols) < cols // 2, 1.0, -1.0)
    return rng.permuted(np.broadcast_to(base, (rows, cols)), axis=1)


def _truncated_normal(rng, shape, bound=3.5):
    """Standard normal samples redrawn until |z| <= bound: at s = 0.031 no output of kind a is
    clipped (3.5 / 0.031 = 113) however many rows and columns the case has."""
    z = rng.standard_normal(shape)
    bad = np.abs(z) > bound
    while bad.any():
        z[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(z) > bound
    return z


def _degenerate_rows(rng, cols):
    u = rng.uniform(-1, 1, size=(4, cols))
    sg = np.where(rng.integers(0, 2, size=(2, cols)) == 1, 1.0, -1.0)
    one_up = np.full(cols, 2.5, np.float32)
    one_up[cols // 2] = np.nextafter(np.float32(2.5), np.float32(3))
    blip = np.zeros(cols, np.float32)
    blip[cols // 3] = 1e-7     # d ~ 1e-7, var ~ 1e-14 / cols << eps: 1 / sqrt(eps) = 1e6 scales the row
    rows = [np.zeros(cols), np.full(cols, -0.0), np.full(cols, 1.5), np.full(cols, -3e4),
            sg[0] * 1e18 * (1 + 0.5 * u[0]), np.zeros(cols), sg[1] * 1e-18 * (1 + 0.5 * u[1]),   # one wave at 768 columns: 4 .. 7
            np.full(cols, 1e18), np.full(cols, -1e-18), one_up, blip, 2 * u[2] + 0.3]
    rows += [np.full(cols, c) for c in rng.standard_normal(8) * 10.0 ** rng.integers(-6, 7, size=8)]
    rows += [np.zeros(cols), np.full(cols, -0.0), 1e18 * u[3], np.zeros(cols)]
    return np.stack([np.asarray(r, np.float64) for r in rows]).astype(np.float32)


@functools.lru_cache(maxsize=8)
def ln_case(c):
    """x [rows][cols], gamma, beta, eps, scale, zp, bw and ref (the reference's int8 bytes)."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    rows, cols = c.rows, c.cols
    eps = float(np.float32(c.eps))
    scale, zp, bw = np.float32(0.031), -3, 8
    finite = None
    if c.kind == "a":
        cs = np.array([A_PARAMS[r % 3] for r in range(rows)])
        x = cs[:, :1] + cs[:, 1:] * _truncated_normal(rng, (rows, cols))
        gamma = 1 + 0.001 * rng.standard_normal(cols)
        beta = 0.001 * rng.standard_normal(cols)
    elif c.kind in ("b", "bm"):
        assert cols % 2 == 0
        x = _signs(rng, rows, cols) * (1 + 1e-4 * rng.uniform(-1, 1, size=(rows, cols)))
        gamma = (-0.75 if c.kind == "bm" else 0.75) * (1 + 2e-5 * rng.uniform(-1, 1, size=cols))
        beta = 0.25 + 1e-5 * rng.uniform(-1, 1, size=cols)
        scale, zp = np.float32(2.0 ** -20), -P20
    elif c.kind == "c":
        assert cols % 2 == 0
        x = _signs(rng, rows, cols) * (2.0 ** (np.arange(rows) % 6 - 2))[:, None]
        # gamma over +-144 / 16: +-gamma / s + beta / s + zp passes either bound for ~6 % of the elements
        gamma = rng.integers(-144, 145, size=cols) / 16.0
        beta = rng.integers(-16, 17, size=cols) / 16.0 + np.where(rng.permutation(cols) % 2 == 0, 1 / 32.0, 0.0)
        scale, zp = np.float32(2.0 ** -4), C_ZP[c.var]
        if abs(zp) >= P20:   # exact: multiples of 1/32 around 2^16 are f32 numbers
            beta = beta - zp * 2.0 ** -4
    elif c.kind in ("d", "f"):
        x = rng.standard_normal((rows, cols)) * 2 + 0.3
        gamma = 1 + 0.05 * rng.standard_normal(cols)
        beta = 0.05 * rng.standard_normal(cols)
        if c.kind == "d":
            bw, zp, s = D_PARAMS[c.var]
            scale = np.float32(s)
            if not 2.0 ** -100 <= s <= 2.0 ** 100:   # y itself at the scale's magnitude: outputs like those at s = 0.031
                gamma, beta = gamma * (s / 0.031), beta * (s / 0.031)
            beta = beta - zp * np.float64(scale)     # values around -zp s: zp + y / s is centred on 0
        else:
            assert rows >= 10 and cols >= 8
            x[1, 5] = np.inf
            x[2, 7] = np.nan
            x[6, cols - 1] = -np.inf
            x[9] = np.nan
            finite = np.isfinite(x).all(axis=1)
    elif c.kind == "e":
        x = _degenerate_rows(rng, cols)
        assert rows == len(x), len(x)
        gamma = 1 + 0.05 * rng.standard_normal(cols)
        beta = rng.standard_normal(cols)
    else:
        raise ValueError(c.kind)
    x, gamma, beta = (np.ascontiguousarray(v, np.float32) for v in (x, gamma, beta))
    if finite is None:
        ref = reference(x, gamma, beta, eps, scale, zp, bw)
    else:
        ref = np.zeros((rows, cols), np.int64)
        ref[finite] = reference(x[finite], gamma, beta, eps, scale, zp, bw)
    lo, hi = (int(v) for v in O.qrange(bw))
    assert ref.min() >= lo and ref.max() <= hi
    d = dict(x=x, gamma=gamma, beta=beta, eps=eps, scale=scale, zp=int(zp), bw=bw, ref=ref.astype(np.int8), finite=finite)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


E_ROWS = 24


def stats(d):
    """Shares of the reference's outputs on either clip bound, and the count of distinct values."""
    lo, hi = (int(v) for v in O.qrange(d["bw"]))
    q = d["ref"] if d["finite"] is None else d["ref"][d["finite"]]
    return dict(at_lo=float((q == lo).mean()), at_hi=float((q == hi).mean()), distinct=int(len(np.unique(q))))


def tie_shares(d):
    """Shares of the elements whose zp + y / s is an unclipped exact half-integer with an even / odd floor."""
    y = O._float_op("LayerNormalization", [O.F(d["x"]), O.F(d["gamma"]), O.F(d["beta"])],
                    {"axis": -1, "epsilon": d["eps"]})[0][1]
    lo, hi = O.qrange(d["bw"])
    u = np.float64(d["zp"]) + (y / d["scale"]).astype(np.float64)
    t = (u - np.floor(u) == 0.5) & (u > lo) & (u < hi)
    return float((t & (np.floor(u) % 2 == 0)).mean()), float((t & (np.floor(u) % 2 == 1)).mean())


# ------------------------------------------------------------------------------- case lists
TREE_COLS = (768, 384, 192)   # 8, 4 and 2 leaves of 96 columns: k_ln_quant_lds / k_ln_quant_reg
GENERIC_COLS = (1, 7, 8, 9, 96, 127, 128, 129, 136, 255, 256, 257, 1024, 1280, 8192)
L = LnCase


def cases_for(cols, kinds="abcdef"):
    """Every case that runs at `cols`: a and d at every width, b at the even widths from 96 up, c
    (balanced signs), e and f where the width allows."""
    out = []
    for eps in EPS:
        if "a" in kinds:
            out.append(L("a", cols, 67, eps))
        if "b" in kinds and cols % 2 == 0 and cols >= 96:
            out += [L("b", cols, 67, eps), L("bm", cols, 67, eps)]
        if "c" in kinds and cols % 2 == 0 and cols >= 96:
            out += [L("c", cols, 67, eps, v) for v in range(len(C_ZP))]
    if "d" in kinds:
        out += [L("d", cols, 67, EPS[v % 2], v) for v in range(len(D_PARAMS))]
    if "e" in kinds:
        out += [L("e", cols, E_ROWS, eps) for eps in EPS]
    if "f" in kinds and cols >= 8:
        out.append(L("f", cols, 67, EPS[0]))
    return out


def case_id(c):
    return "-".join(str(v) for v in c)
