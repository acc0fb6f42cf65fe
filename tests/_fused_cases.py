"""Inputs of tests/test_gpu_fused_reference.py and their references (tests/_fused_ref.py), built on
the host from NumPy alone so that the input conditions — accumulators that reach the
f32-exactness bound, exact rounding ties, unclipped outputs, softmax rows of a stated kind — are
asserted on the reference itself (tests/test_fused_ref_inputs.py runs them without a GPU).
Every builder is cached: one reference per case, shared by all kernel routes, never modified."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import _fused_ref as R
import _ln_cases
from oracle import nq_oracle as O

GemmCase = namedtuple("GemmCase", "epi M N K kind bw zpa zpo wbits l1", defaults=("rand", 8, -5, "std", 8, False))
T_TOK, DH = 197, 64
ZPO = {"p100": 100, "0": 0, "p20": 1 << 20, "m20": -(1 << 20), "p20+1": (1 << 20) + 1, "m20-1": -(1 << 20) - 1}
F32_LIMIT = 1 << 24


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, list):
            for x in v:
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
    return d


def _extreme_operands(c, rng):
    """Weights and rows that realise the f32-exactness bound abound + cmax |zpa| exactly
    (nqk_qgemm_fused: abound = 2^14 K, or 128 col_l1max when the caller gives it).
    K = 768: full-range weights, every 64th column all -128 (cmax = 128 K); K = 3072: weights in
    [-42, 42], every 64th column all +42 (col_l1max = cmax = 42 K).  Rows 0 / M - 1 are all -128:
    with zpa > 0 their |acc - col zpa| in those columns IS the bound (an even number).  Columns
    64 j + 1 hold the odd constant next to it (-127 / +41) and rows 1 / M - 2 are all -127 but for
    one -128: an odd |acc - col zpa| within 5 % of the bound.  Columns 64 j + 2 alternate in sign;
    rows 2, 3: a = -128 where b > 0, 127 where b < 0, and the mirror image."""
    M, N, K = c.M, c.N, c.K
    w = 42 if c.l1 else 128
    bt = rng.integers(-w, w + (0 if w == 128 else 1), size=(N, K)).astype(np.int64)
    lead = w if c.l1 else -w
    bt[0::64] = lead
    bt[1::64] = 41 if c.l1 else -127
    alt = np.where(np.arange(K) % 2 == 0, np.clip(w, -128, 127), -w)
    bt[2::64] = alt
    a = rng.integers(-128, 128, size=(M, K)).astype(np.int64)
    a[0] = a[M - 1] = -128
    a[1] = a[M - 2] = -127
    a[1, -1] = a[M - 2, -1] = -128
    a[2] = np.where(alt > 0, -128, 127)
    a[3] = np.where(alt > 0, 127, -128)
    rows = np.array([0, 1, 2, 3, M - 2, M - 1])
    return a.astype(np.int8), bt.astype(np.int8), rows


@functools.lru_cache(maxsize=3)
def gemm_case(c):
    """Host operands, epilogue scalars, the reference outputs and the measured input conditions."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    M, N, K = c.M, c.N, c.K
    ng = 3 if c.epi == "qkv" else 1
    stats, rows = {}, None
    ln_rows = _ln_rows_case(c) if c.kind.startswith("rows_") else None
    if c.kind == "extreme":
        a, bt, rows = _extreme_operands(c, rng)
    elif ln_rows is not None:  # a = 0, zpa = 0, no bias: the epilogue's f32 row is the residual row exactly
        assert c.epi == "resid_ln" and c.zpa == 0 and c.bw == 8
        a = np.zeros((M, K), np.int8)
        bt = rng.integers(-24, 25, size=(N, K)).astype(np.int8)
    else:
        wl = 8 if (c.wbits == 4 or c.kind == "ties") else 24
        a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
        bt = rng.integers(-wl, wl + (0 if c.wbits == 4 else 1), size=(N, K)).astype(np.int8)
    col = bt.astype(np.int64).sum(axis=1)
    l1 = int(np.abs(bt.astype(np.int64)).sum(axis=1).max())
    cmax = int(np.abs(col).max())
    zp_std = (3, -140, 0) if c.bw == 8 else (1, -1, 0)
    zp_out = [ZPO[c.zpo] if c.zpo != "std" else zp_std[g] for g in range(3)]
    if c.kind == "extreme":
        s_acc = [np.float32(1e-6)] * 3
        s_out = [np.float32(0.14 * 2 ** (8 - c.bw))] * 3
    elif c.kind == "ties":
        s_acc = [np.float32(2.0 ** -13)] * 3
        s_out = [np.float32(2.0 ** -6)] * 3
        zp_out = [3, -4, 0]
    else:
        # dequantized values of standard deviation ~2: var(v) = K E[(a - zpa)^2] E[w^2]
        sw2 = float((bt.astype(np.float64) ** 2).mean())
        sd = np.sqrt(K * (74.0 ** 2 + (0.5 + c.zpa) ** 2) * sw2)
        s_acc = [np.float32(2.0 / sd * (1 + 0.1 * g)) for g in range(3)]
        base = (0.011, 0.0173, 0.05) if c.epi == "qkv" else ({"small": 0.0027, "tiny": 0.0008}.get(c.kind, 0.0125),) * 3
        s_out = [np.float32(base[g]) for g in range(3)]
        if c.bw < 8:  # a few units of standard deviation 2 across the narrow range
            s_out = [np.float32(6.0 / 2 ** c.bw * (1 + 0.3 * g)) for g in range(3)]
    G = N // ng
    bias = (0.05 * rng.standard_normal(N)).astype(np.float32)
    if c.kind == "ties":
        bias = (rng.integers(-2000, 2001, size=N) * np.float64(s_acc[0])).astype(np.float32)
    for g in range(ng):  # a large output zero point: values around -zp s_out, so that outputs are not all clipped
        if abs(zp_out[g]) >= 1 << 20:
            bias[g * G:(g + 1) * G] += np.float32(-zp_out[g] * np.float64(s_out[g]))
    res = rng.standard_normal((M, N)).astype(np.float32) if c.epi in ("resid", "resid_ln") else None
    if ln_rows is not None:
        bias, res = np.zeros(N, np.float32), ln_rows["x"]
    d = dict(a=a, bt=bt, col=col, bias=bias, resid=res, s_acc=s_acc, s_out=s_out, zp_out=zp_out, col_absmax=cmax,
             col_l1max=l1 if c.l1 else 0, heads=G // DH if c.epi == "qkv" else 0)
    lo, hi = O.qrange(c.bw)
    if c.epi == "qkv":
        d["ref"] = R.qkv(a, bt, bias, c.zpa, s_acc, s_out, zp_out, c.bw, T_TOK, d["heads"], DH)
    elif c.epi == "resid":
        d["ref"] = [R.resid(a, bt, bias, res, c.zpa, s_acc[0])]
    elif ln_rows is not None:
        d.update(gamma=ln_rows["gamma"], beta=ln_rows["beta"], ln_scale=ln_rows["scale"], ln_zp=ln_rows["zp"],
                 ln_eps=ln_rows["eps"], ln_case=ln_rows)
        y, q = R.resid_ln(a, bt, bias, res, c.zpa, s_acc[0], d["gamma"], d["beta"], d["ln_eps"], d["ln_scale"], d["ln_zp"], c.bw)
        assert np.array_equal(y.view(np.int32), res.view(np.int32)) and np.array_equal(q, ln_rows["ref"])
        d["ref"] = [y, q]
    elif c.epi == "resid_ln":
        d["gamma"] = (1 + 0.1 * rng.standard_normal(N)).astype(np.float32)
        d["beta"] = (0.1 * rng.standard_normal(N)).astype(np.float32)
        d["ln_scale"] = np.float32(0.021 * 2 ** (8 - c.bw))
        d["ln_zp"] = ZPO[c.zpo] if c.zpo != "std" else {8: -5, 3: 1, 2: 0}[c.bw]
        d["ln_eps"] = float(np.float32(1e-12))
        if abs(d["ln_zp"]) >= 1 << 20:
            d["beta"] = d["beta"] + np.float32(-d["ln_zp"] * np.float64(d["ln_scale"]))
        y, q = R.resid_ln(a, bt, bias, res, c.zpa, s_acc[0], d["gamma"], d["beta"], d["ln_eps"], d["ln_scale"], d["ln_zp"],
                          c.bw)
        d["ref"] = [y, q]
        stats["clipped"] = float(((q == lo) | (q == hi)).mean())
        assert stats["clipped"] < 0.5, stats
    else:
        d["ref"] = [R.gelu(a, bt, bias, c.zpa, s_acc[0], s_out[0], zp_out[0], c.bw).astype(np.int8)]
        stats["clipped"] = float(((d["ref"][0] == lo) | (d["ref"][0] == hi)).mean())
        if c.kind == "tiny":  # the scale without a GELU table: the filtered chain decides most outputs unclipped
            assert stats["clipped"] < 0.5, stats
    if c.kind == "extreme":
        # the accumulators of the extreme rows reach the bound of the f32-exactness proof exactly
        v = a[rows].astype(np.int64) @ bt.astype(np.int64).T - col[None, :] * c.zpa
        abound = min(16384 * K, 128 * l1) if c.l1 else 16384 * K
        bound = abound + cmax * abs(c.zpa)
        stats.update(vmax=int(np.abs(v).max()), bound=bound, below=bound < F32_LIMIT,
                     parities=sorted(set((np.abs(v[np.abs(v) > 0.95 * bound]) & 1).tolist())))
        assert c.zpa > 0 and stats["vmax"] == bound and stats["parities"] == [0, 1], stats
        if c.epi != "resid":  # the extreme rows' outputs are not all clipped
            if c.epi == "qkv":
                q = np.concatenate(R.qkv(a[rows], bt, bias, c.zpa, s_acc, s_out, zp_out, c.bw, T_TOK, d["heads"], DH, False), 1)
            else:
                q = d["ref"][0][rows].astype(np.int64)
            stats["clipped"] = float(((q == lo) | (q == hi)).mean())
            assert stats["clipped"] < 0.5, stats
    if c.kind == "ties":
        ties = even = odd = 0
        for g in range(3):
            y = R._biased(a, bt, c.zpa, s_acc[g], bias, slice(g * G, (g + 1) * G))
            u = np.float64(zp_out[g]) + (y / s_out[g]).astype(np.float64)
            t = (u - np.floor(u) == 0.5) & (u > lo) & (u < hi)
            ties += int(t.sum())
            even += int((t & (np.floor(u) % 2 == 0)).sum())
            odd += int((t & (np.floor(u) % 2 == 1)).sum())
        stats.update(tie_share=ties / (M * N), even=even, odd=odd)
        assert stats["tie_share"] >= 0.005 and even > 0 and odd > 0, stats
    d["stats"] = stats
    return _freeze(d)


def _ln_rows_case(c):
    """The LayerNorm case (tests/_ln_cases.py, 192 columns) whose rows are the residual of a
    "rows_<kind>" case; a trailing 5 in the kind selects eps = 1e-5 instead of 1e-12."""
    kind = c.kind[len("rows_"):]
    eps = _ln_cases.EPS[1] if kind.endswith("5") else _ln_cases.EPS[0]
    assert c.N == 192
    return _ln_cases.ln_case(_ln_cases.LnCase(kind.rstrip("5"), c.N, c.M, eps))


# ------------------------------------------------------------------------------- attention
AttnCase = namedtuple("AttnCase", "T zset sp bw", defaults=(8,))
ZSETS = {"std": (-5, 3, None, 2), "fast": (380, -380, None, 180), "lim+": (4096, -4096, 1024, -1024), "lim-": (-4096, 4096, -1024, 1024),
         "limqk": (4096, 4096, None, 1024)}
SP = {"unit": (1.0 / 255, -128), "cal": (8e-5, -142)}
B_ATT, H_ATT = 2, 3
SWITCH = -86.5  # the exponent-add exp variant's switch point (nqk_selftest_fastmath)


def _attn_operands(c, s_p=None):
    """q, k, v [6][T][64] with, per (batch, head): 0 random; 1 flat softmax rows (all keys equal);
    2 peaked rows (one key ahead by more than 104: every other exp is 0); 3 rows whose softmax
    arguments straddle -86.5; 4 all -128; 5 all 127.  s_qk is chosen so that the graded keys of
    head 3 are 0.85 apart in score.  With them the reference scores, P and its row sums, and the
    measured row conditions."""
    T = c.T
    zq, zk, zp_p, zv = ZSETS[c.zset]
    s_p, zp_sp = (SP[c.sp][0] if s_p is None else s_p), SP[c.sp][1]   # (s_p given: attn_sum_case)
    zp_p = zp_sp if zp_p is None else zp_p
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    lo, hi = (int(x) for x in O.qrange(c.bw))  # q, k, v hold bit_width-bit values (lo = -128, hi = 127 at 8)
    q, k, v = (rng.integers(lo, hi + 1, size=(B_ATT * H_ATT, T, DH)).astype(np.int8) for _ in range(3))
    cq = hi if zq <= 0 else lo             # the query value of largest |q - zq|
    up = hi if cq - zq > 0 else lo         # the key value that raises the score
    k[1] = rng.integers(lo, hi + 1, size=(1, DH))
    q[2], k[2] = cq, lo + hi - up          # every key at the lowering value (hi <-> lo) but one
    k[2][T // 2] = up
    q[3] = cq
    grade = np.clip(up - np.sign(up) * np.arange(T), lo, hi)
    k[3] = rng.permutation(grade)[:, None]
    q[4], k[4], v[4] = lo, lo, lo
    q[5], k[5], v[5] = hi, hi, hi
    s_qk = np.float32(0.85 * 8.0 / (DH * abs(cq - zq)))
    div = 8.0
    stats = {}
    s = R.scores(q, k, zq, zk, s_qk, div)
    p, psum = R.softmax_quant(s, (T + 15) // 16 * 16, s_p, zp_p, c.bw)
    if T >= 16 and c.bw == 8:
        arg = s + (-s.max(axis=-1, keepdims=True))
        assert (arg[1] == 0).all()                                   # flat
        second = np.sort(arg[2], axis=-1)[:, -2]
        stats["peak_gap"] = float(-second.max())
        assert stats["peak_gap"] > 104                               # peaked
        stats["straddle"] = (int(((arg[3] > SWITCH) & (arg[3] < SWITCH + 2)).sum()),
                             int(((arg[3] < SWITCH) & (arg[3] > SWITCH - 2)).sum()))
        if T >= 197:
            assert stats["straddle"][0] > 0 and stats["straddle"][1] > 0, stats
    return dict(q=q, k=k, v=v, zq=zq, zk=zk, zp_p=zp_p, zv=zv, s_qk=s_qk, div=div, s_p=np.float32(s_p), scores=s, p=p,
                psum=psum, stats=stats)


@functools.lru_cache(maxsize=4)
def attn_case(c):
    """The operands of _attn_operands with a calibrated-looking context scale, and the reference of
    every stage: scores, P and its row sums, V^T and its sums, the context."""
    return _freeze(_attn_finish(c, _attn_operands(c)))


def _attn_finish(c, d):
    T = c.T
    q, k, v, p, zq, zk, zp_p, zv, s_qk, div, s_p, stats = (d[x] for x in "q k v p zq zk zp_p zv s_qk div s_p stats".split())
    lo, hi = (int(x) for x in O.qrange(c.bw))
    s_v = np.float32(0.043)
    s_pv = np.float32(s_p * s_v)
    # a calibrated-looking context scale: the dequantized P.V values fill the int8 range
    acc, z = R._full_acc(p[..., :T], v, zp_p, zv, T)
    dctx = O.dequantize(acc, s_pv, z)
    s_ctx = np.float32(max(np.abs(dctx).max(), 1e-3) / (0.47 * (hi - lo)))
    zp_ctx = int(-np.rint((dctx.max() + dctx.min()) / 2 / s_ctx))
    ctx = R.pv(p, v, zp_p, zv, s_pv, s_ctx, zp_ctx, c.bw, H_ATT, T)
    stats["ctx_clipped"] = float(((ctx == lo) | (ctx == hi)).mean())
    assert np.array_equal(ctx, R.attention(q, k, v, H_ATT, zq, zk, s_qk, div, s_p, zp_p, s_pv, zv, s_ctx, zp_ctx, c.bw))
    vt, vsum = R.transpose_pad(v, (T + 15) // 16 * 16)
    return dict(d, s_pv=s_pv, s_ctx=s_ctx, zp_ctx=zp_ctx, vt=vt, vsum=vsum, ctx=ctx)


@functools.lru_cache(maxsize=2)
def attn_sum_case(T, sign):
    """AttnCase(T, "std", "unit") with s_p moved from 1 / 255 by a few thousand f32 steps, to where
    the LAST BIT of the softmax denominator shows in the context.  (With s_p = 1 / 255 or 8e-5 it does
    not: summing a row of exps in another pairwise order changes the denominator of 8 .. 26 % of the
    rows by one ulp and not one P.)  The rows of head 3 are identical (one query value, graded keys in
    a random order: a sum with roundoff).  s_p is the f32 value nearest 1 / 255 at which the row's
    largest probability (of those the neighbour changes) quantizes differently for the denominator and for its neighbour one ulp
    above (sign = +1) or below (-1); asserted on the reference: with that neighbour as the
    denominator of head 3, P changes in every row and the context in at least T elements."""
    c = AttnCase(T, "std", "unit")
    s = _attn_operands(c)["scores"][3, 0]
    ex = np.exp(s + (-s.max()))
    den = ex.sum()
    assert ex.dtype == np.float32 and den.dtype == np.float32
    alt = np.nextafter(den, np.float32(np.inf * sign))
    base = np.float32(1.0 / 255).view(np.int32)
    cand = (base + np.arange(-200000, 200001, dtype=np.int32)).view(np.float32)
    zp, s_p = np.int64(SP["unit"][1]), None
    for j in np.argsort(-ex)[:8]:  # the largest probability that the neighbour changes at all
        p_ref, p_alt = ex[j] / den, ex[j] / alt
        hit = np.flatnonzero(O.quantize(p_ref / cand, 8, np.float32(1), zp) != O.quantize(p_alt / cand, 8, np.float32(1), zp))
        if p_ref != p_alt and hit.size:
            s_p = cand[hit[np.abs(hit - 200000).argmin()]]
            break
    assert s_p is not None, "no scale within 200 000 steps of 1 / 255 puts one of the 8 largest probabilities on a boundary"
    d = _attn_finish(c, _attn_operands(c, s_p=s_p))
    assert np.array_equal(d["p"][3, 0, :T], O.quantize(ex / den, 8, s_p, zp))  # the oracle's Softmax, restated
    p2 = d["p"].copy()
    p2[3, :, :T] = O.quantize(ex / alt, 8, s_p, zp)
    ctx2 = R.pv(p2, d["v"], d["zp_p"], d["zv"], d["s_pv"], d["s_ctx"], d["zp_ctx"], 8, H_ATT, T)
    d["stats"].update(s_p_steps=int(s_p.view(np.int32)) - int(base), p_changed=int((p2 != d["p"]).sum()),
                      ctx_changed=int((ctx2 != d["ctx"]).sum()))
    assert d["stats"]["p_changed"] >= T and d["stats"]["ctx_changed"] >= T, d["stats"]
    return _freeze(d)


EXACT_T = (577, 1618)  # 1618: the most tokens nqk_attention_long's int32 bound admits at |zp_p| = |zv| = 1024


@functools.lru_cache(maxsize=2)
def attn_exact_case(T, zset):
    """The int32 zero-point algebra of the context at the zero-point limits (zset "lim+" / "lim-",
    the operands of _attn_operands), resolved to one part in 2^(31 - e): with s_pv = 2^-13 and
    s_ctx = 2^(e - 13) the context is zp_ctx + (acc - z) / 2^e exactly, one step per 2^e int32 units,
    centred on the median of acc - z over the four heads with random V (zp_ctx).  e is the smallest
    integer at which under 2 % of those heads' reference context is clipped; they must then hold
    at least 64 distinct values.  (With |zp_p| = 1024 every P clamps to 127 or -128, so the context
    of a head varies over its 64 dimensions only: 256 values at the most.)"""
    assert zset in ("lim+", "lim-")
    d = _attn_operands(AttnCase(T, zset, "unit"))
    p, v, zp_p, zv = d["p"], d["v"], d["zp_p"], d["zv"]
    s_pv = np.float32(2.0 ** -13)
    acc, z = R._full_acc(p[..., :T], v, zp_p, zv, T)
    w = acc - z
    stats = dict(d["stats"], acc_absmax=int(np.abs(w).max()))
    assert stats["acc_absmax"] < 1 << 31, stats
    med = float(np.median(w[:4]))
    for e in range(31):
        s_ctx = np.float32(2.0 ** (e - 13))
        zp_ctx = int(-np.rint(med / 2.0 ** e))
        c4 = O.quantize(O.dequantize(acc[:4], s_pv, z[:4]), 8, s_ctx, np.int64(zp_ctx))
        clip = float(((c4 == -128) | (c4 == 127)).mean())
        if clip < 0.02:
            break
    stats.update(e=e, clip_share=clip, distinct=int(len(np.unique(c4))))
    assert stats["clip_share"] < 0.02 and stats["distinct"] >= 64, stats
    ctx = R.pv(p, v, zp_p, zv, s_pv, s_ctx, zp_ctx, 8, H_ATT, T)
    q, k = d["q"], d["k"]
    assert np.array_equal(ctx, R.attention(q, k, v, H_ATT, d["zq"], d["zk"], d["s_qk"], d["div"], d["s_p"], zp_p, s_pv, zv,
                                           s_ctx, zp_ctx, 8))
    return _freeze(dict(q=q, k=k, v=v, zq=d["zq"], zk=d["zk"], zp_p=zp_p, zv=zv, s_qk=d["s_qk"], div=d["div"], s_p=d["s_p"],
                        s_pv=s_pv, s_ctx=s_ctx, zp_ctx=zp_ctx, ctx=ctx, stats=stats))


@functools.lru_cache(maxsize=1)
def pv_ties_case():
    """EPI_PV on exact ties: power-of-two scales (2^-13, 2^-6), so zp + d / s_ctx = zp + v / 128 is a
    half-integer whenever v = 64 (mod 128)."""
    T, Tp = T_TOK, 208
    rng = np.random.default_rng(99)
    p = np.zeros((B_ATT * H_ATT, T, Tp), np.int8)
    p[..., :T] = rng.integers(-16, 17, size=(B_ATT * H_ATT, T, T))
    v = rng.integers(-16, 17, size=(B_ATT * H_ATT, T, DH)).astype(np.int8)
    zp_p, zv, s_pv, s_ctx, zc = -3, 2, np.float32(2.0 ** -13), np.float32(2.0 ** -6), 3
    acc, z = R._full_acc(p[..., :T], v, zp_p, zv, T)
    u = np.float64(zc) + (O.dequantize(acc, s_pv, z) / s_ctx).astype(np.float64)
    t = (u - np.floor(u) == 0.5) & (u > -128) & (u < 127)
    stats = dict(tie_share=float(t.mean()), even=int((t & (np.floor(u) % 2 == 0)).sum()),
                 odd=int((t & (np.floor(u) % 2 == 1)).sum()))
    assert stats["tie_share"] >= 0.005 and stats["even"] > 0 and stats["odd"] > 0, stats
    ctx = R.pv(p, v, zp_p, zv, s_pv, s_ctx, zc, 8, H_ATT, T)
    return _freeze(dict(p=p, v=v, vt=R.transpose_pad(v, Tp)[0], zp_p=zp_p, zv=zv, s_pv=s_pv, s_ctx=s_ctx, zp_ctx=zc, ctx=ctx,
                        stats=stats))


# ------------------------------------------------------------------------------- case lists
C = GemmCase
_FB = ["epi", "big", "pg_fb", "proj_fb"]   # *_fb: the persistent kernels are offered the case and must decline it
_F32 = ["epi", "big", "pg", "proj"]

# every route at the smallest shapes that reach it (input 4: random data, small output scales)
ROUTE_CASES = [
    (C("qkv", 131, 192, 192, "small"), ["epi", "big", "big_pack", "pg"]),
    (C("qkv", 197 * 3, 576, 192, "small"), ["epi", "big", "big_pack", "pg"]),
    # (k_proj takes whole images only, M % tokens == 0: it must decline the partial last image, proj_fb)
    (C("qkv", 300, 768, 768, "small"), ["epi", "big", "big_pack", "proj_fb", "pg", "pg_wm2"]),
    (C("qkv", 256 + 77, 2304, 768, "small"), ["big", "proj_fb", "pg", "pg_wm2"]),
    (C("qkv", 197 * 2, 768, 768, "small"), ["big", "proj", "pg_wm2"]),
    (C("qkv", 197 * 2, 2304, 768, "small"), ["proj", "pg"]),
    (C("qkv", 197 * 3, 576, 3072, "small"), ["epi", "big"]),
    (C("resid", 131, 768, 192), ["epi", "big", "big_pack", "pg"]),
    (C("resid", 300, 768, 768), ["epi", "big", "big_pack", "pg", "pg_wm2"]),
    (C("resid", 512, 768, 768), ["proj", "pg_wm2"]),
    (C("resid", 256 + 77, 768, 3072, l1=True), ["big", "pg", "pg_wm2"]),
    (C("resid", 256, 768, 3072, l1=True), ["proj", "pg"]),
    (C("resid", 131, 3072, 192), ["big", "pg"]),
    (C("gelu", 131, 768, 192), ["epi", "big", "big_pack", "pg", "glut"]),
    (C("gelu", 300, 3072, 768, "small"), ["big", "big_pack", "proj", "pg", "pg_wm2", "glut", "glut_wm2"]),
    (C("gelu", 197 * 3, 768, 768, "small"), ["epi", "pg", "glut"]),
    # s_out = 0.0008: the increasing branch alone needs > 1024 buckets of 0.885 s, so nqk_gelu_lut_build
    # returns n = 0; zp_out = 100 keeps the negative half of the GELU outputs unclipped
    (C("gelu", 300, 768, 768, "tiny", zpo="p100"), ["nolut"]),
    (C("gelu", 131, 2304, 3072), ["big"]),
]
# input 3: bit widths, output zero points, zpa
for _bw in (2, 3):
    ROUTE_CASES += [(C("qkv", 197 * 2, 768, 768, bw=_bw), ["epi", "big", "pg", "proj"]),
                    (C("gelu", 300, 768, 768, bw=_bw), ["epi", "big", "pg"])]
for _bw in (2, 3, 4):
    ROUTE_CASES += [(C("qkv", 300, 768, 768, bw=_bw, wbits=4), ["big_pack4", "pg4"]),
                    (C("gelu", 300, 768, 768, bw=_bw, wbits=4), ["big_pack4", "pg4"])]
ROUTE_CASES += [(C("resid", 300, 768, 768, bw=4, wbits=4), ["big_pack4", "pg4"]),
                (C("resid", 300, 768, 3072, bw=4, wbits=4), ["big_pack4", "pg4"])]
for _e, _m in (("qkv", 197 * 2), ("gelu", 300)):  # QKV: two whole images (k_proj), ragged against 128 and 256 rows
    for _z in ("0", "p20", "m20"):
        ROUTE_CASES.append((C(_e, _m, 768, 768, zpo=_z), _F32))
    for _z in ("p20+1", "m20-1"):
        ROUTE_CASES.append((C(_e, _m, 768, 768, zpo=_z), _FB))
for _e, _m in (("qkv", 197 * 2), ("gelu", 300), ("resid", 300)):
    for _z in (0, -128, 127):
        ROUTE_CASES.append((C(_e, _m, 768, 768, zpa=_z), ["epi", "big", "pg"] + (["proj"] if _e != "resid" else [])))
    ROUTE_CASES.append((C(_e, _m, 768, 768, zpa=1 << 20), ["epi", "big", "big_pack"]))

# input 1: accumulators at the f32-exactness bound, just below 2^24 and just above
EXTREME_CASES = []
for _z in (40, 43, 140):  # K = 768 without col_l1max: 2^14 K + 128 K zpa = 16 515 072 / 16 809 984 / 26 345 472
    _lo = _z == 40
    EXTREME_CASES += [(C("qkv", 131, 576, 768, "extreme", zpa=_z), ["epi", "big", "pg" if _lo else "pg_fb"]),
                      (C("gelu", 131, 768, 768, "extreme", zpa=_z), ["epi", "big", "pg" if _lo else "pg_fb"]),
                      (C("resid", 256, 768, 768, "extreme", zpa=_z), ["big", "pg", "pg_wm2", "proj"])]
for _z in (2, 3):  # K = 3072 with col_l1max = 42 K: 128 L + L zpa = 16 773 120 / 16 902 144
    EXTREME_CASES += [(C("resid", 256, 768, 3072, "extreme", zpa=_z, l1=True), ["big", "pg", "pg_wm2", "proj"]),
                      (C("qkv", 131, 576, 3072, "extreme", zpa=_z, l1=True), ["big"]),
                      (C("gelu", 131, 768, 3072, "extreme", zpa=_z, l1=True), ["big"])]

# input 2: exact ties
TIES_CASES = [(C("qkv", 197 * 3, 576, 192, "ties"), ["epi", "big", "big_pack", "pg"]),
              (C("qkv", 197 * 2, 768, 768, "ties"), ["big", "pg", "pg_wm2", "proj"])]

# the fused LayerNorm of k_qgemm_big at N = 192: bit widths, ln_zp at +-2^20 (magic-number quantize) and beyond (f64)
LN_CASES = [(C("resid_ln", 197 * 3, 192, 192, bw=_bw), ["big", "big_pack"]) for _bw in (2, 3, 8)]
LN_CASES += [(C("resid_ln", 131, 192, 768, zpo=_z), ["big", "big_pack"]) for _z in ("0", "p20", "m20", "p20+1", "m20-1")]

# the same kernel on residual rows whose int8 bytes see the last bit of the mean, the variance, 1 / sqrt and the last
# multiply-add (tests/_ln_cases.py kinds a, b, bm, c), with both epsilons
LN_ROW_CASES = [(C("resid_ln", 131, 192, 192, "rows_" + _k, zpa=0), ["big", "big_pack"])
                for _k in ("a", "a5", "b", "b5", "bm", "bm5", "c", "c5")]

# persistent routes: some workgroup walks >= 3 tiles and the last row tile is ragged (see the test's docstring)
PERSIST_CASES = [(C("gelu", 1024 * 128 + 77, 64, 192, "small"), ["pg"]),
                 (C("gelu", 512 * 256 + 77, 64, 768, "small"), ["pg_wm2"]),
                 (C("gelu", 16 * 256 + 77, 256, 768, "small"), ["proj8"])]

A = AttnCase
ATTN_CASES = [A(T, "std", sp) for T in (1, 16, 17, 197, 224) for sp in ("unit", "cal")]
ATTN_CASES += [A(T, z, "unit") for z in ("lim+", "lim-", "limqk") for T in (17, 197)]
ATTN_CASES += [A(197, "fast", sp) for sp in ("unit", "cal")]
ATTN_CASES += [A(17, "std", "unit", _bw) for _bw in (2, 3)]

# nqk_attention_long (225 .. 1856 tokens), each T the smallest at an edge of k_attn_long or of NumPy's
# pairwise sum: 225 the first it takes (TP = 256: one key in the last 16-key score tile, one row in
# the last query block); 256 | 257, 512 | 513, 1025 the pairwise-sum depths (257: five 64-key chunks,
# 1025: seventeen, an odd count in the two-accumulator P V loop); 640 | 641 the 64 KiB default of
# dynamic LDS (80 TP + 10 880 = 62 080 | 67 200 bytes); 1856 the last it takes.  (577 with the
# limit zero points of Q and K: the ViT/16 count at 384 px.)  attn_case keeps four cases: the list
# ascends in T and the stage list below descends, so a test over the one followed by a test over the
# other finds the costly references (1856 and 1025 tokens: 2.5 and 0.5 s) still cached; every
# reference below 641 tokens builds in under 0.2 s.
LONG_T = (225, 256, 257, 512, 513, 640, 641, 1025, 1856)
LONG_ATTN_CASES = []
for _T in LONG_T:
    LONG_ATTN_CASES += [A(_T, "std", sp) for sp in ("unit", "cal")]
    if _T == 257:
        LONG_ATTN_CASES += [A(257, "limqk", "unit")] + [A(257, "std", "unit", _bw) for _bw in (2, 3, 4)]
    if _T == 513:
        LONG_ATTN_CASES += [A(577, "limqk", "unit")]
# the softmax denominator's last bit (attn_sum_case), at every depth of the pairwise sum
SUM_T = (225, 257, 513, 1025)   # one, two, three and four splits
# the three-launch chain past 224 tokens, stage by stage
LONG_STAGE_CASES = [A(_T, "std", "cal") for _T in (1856, 1025, 641, 257, 225)] + [A(577, "limqk", "unit")]
