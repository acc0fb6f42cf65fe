"""nqk_attention_long (225 .. 1856 tokens) and the three-launch chain at these lengths against the
plain NumPy reference (tests/_fused_ref.py, pinned to the oracle's node loop at 197 and 226 tokens
by tests/test_fused_ref.py).  tests/test_gpu_attention_long.py compares the kernel with the chain,
another HIP path that shares row_plan / wave_pairwise_sum, np_expf and copies of div_rc / quant_zp
with it; here neither side is the other's reference.  Every comparison is bit for bit.

The inputs are the rows the 197-token cases were built around (tests/_fused_cases.py attn_case:
per head random, flat, peaked by more than 104, straddling -86.5, all -128, all 127), at the token
counts on k_attn_long's edges (LONG_ATTN_CASES), and attn_exact_case: the zero-point limits with
power-of-two scales, where one context step is 2^15 (577 tokens) or 2^16 (1618 tokens, the most the
int32 bound admits) of accumulators that reach 1.67e9; and attn_sum_case: a softmax scale at which
the last bit of the softmax denominator decides the context."""
import ctypes

import numpy as np
import pytest

import _fused_cases as F
from _fused_gpu import attn_params, check_three_launch_pieces, head_mismatches

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
BH, H, DH = F.B_ATT * F.H_ATT, F.H_ATT, F.DH


def _id(c):
    return "-".join(map(str, c))


def _upload(d, T):
    from numpy_quant.device import DeviceArray
    return [DeviceArray.from_host(d[x].reshape(BH * T, DH)) for x in "qkv"]


def _long(d, T, bw, q_rows=0, ld_out=None):
    """nqk_attention_long on the case's operands into a sentinel-filled ctx [B][T][ld_out]."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    dq, dk, dv = _upload(d, T)
    a = attn_params(d, H, T, bw)
    a.q_rows = q_rows
    if ld_out is not None:
        a.ld_out = ld_out
    ctx = DeviceArray.from_host(np.full((F.B_ATT, T, a.ld_out), SENTINEL, dtype=np.int8))
    _lib.call("nqk_attention_long", dq.vp, dk.vp, dv.vp, ctx.vp, BH, ctypes.byref(a))
    return ctx.to_host()


def _equal(got, want, T):
    assert int((got != want).sum()) == 0, head_mismatches(got, want, T)


@pytest.mark.parametrize("case", F.LONG_ATTN_CASES, ids=_id)
def test_long_attention_equals_the_reference(case):
    """Every token count on an edge of k_attn_long (tests/_fused_cases.py LONG_ATTN_CASES) with both
    softmax scales, the limit zero points of Q and K at 257 and 577, bit widths 2, 3 and 4 at 257."""
    d = F.attn_case(case)
    _equal(_long(d, case.T, case.bw), d["ctx"], case.T)


@pytest.mark.parametrize("zset", ["lim+", "lim-"])
@pytest.mark.parametrize("T", F.EXACT_T)
def test_long_attention_int32_algebra_at_the_limits(T, zset):
    """(zq, zk, zp_p, zv) = +-(4096, -4096, 1024, -1024) with a context step of 2^e int32 units
    (attn_exact_case: e = 15 at 577 tokens, 16 at 1618; under 2 % clipped, 126 .. 145 distinct values
    in the heads with random V).  At 1618 tokens |acc - z| reaches 1 670 499 246 of 2^31 in the
    all -128 / all 127 heads."""
    d = F.attn_exact_case(T, zset)
    _equal(_long(d, T, 8), d["ctx"], T)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("T", F.SUM_T)
def test_long_attention_softmax_denominator_to_the_last_bit(T, sign):
    """With s_p = 1 / 255 or 8e-5 a softmax denominator that is one ulp off changes no P on these
    inputs (measured on the reference), so the cases above would pass a pairwise sum taken in another
    order.  attn_sum_case moves s_p to where the neighbouring denominator (one ulp above | below)
    changes P in every row of head 3 and the context in 4112 .. 12 300 elements, at each depth of
    NumPy's pairwise sum (one split up to 256 elements, two up to 512, three up to 1024, four above)."""
    d = F.attn_sum_case(T, sign)
    _equal(_long(d, T, 8), d["ctx"], T)


def test_long_attention_refuses_one_token_past_the_int32_bound():
    """1618 * (16384 + 128 * 2048 + 1024 * 1024) = 2 147 254 272 < 2^31 is taken (the test above),
    1619 * 1 327 104 = 2 148 581 376 is refused, by the entry point and by the plan's predicate."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.plan import attn_long_accepts
    d = F.attn_exact_case(1618, "lim+")  # (cached by the test above)
    zq, zk, zp, zv = (d[x] for x in ("zq", "zk", "zp_p", "zv"))
    scales = (d["s_qk"], d["div"], d["s_p"], d["s_pv"], d["s_ctx"])
    assert attn_long_accepts(1618, DH, 8, zq, zk, zp, zv, scales)
    assert not attn_long_accepts(1619, DH, 8, zq, zk, zp, zv, scales)
    assert attn_long_accepts(1619, DH, 8, zq, zk, zp, zv + 1, scales)  # the bound, not the token count
    bufs = [DeviceArray((BH * 1619, DH), np.int8) for _ in range(4)]   # a refusal that went missing would launch in bounds
    a = attn_params(d, H, 1619, 8)
    with pytest.raises(_lib.NQKError, match="int32-exact range at this token count"):
        _lib.call("nqk_attention_long", *[b.vp for b in bufs], BH, ctypes.byref(a))


@pytest.mark.parametrize("case", F.LONG_STAGE_CASES, ids=_id)
def test_three_launch_pieces_equal_the_reference_past_224_tokens(case):
    """nqk_transpose_pad_i8 (with its int64 sums), EPI_SCORES at N = T, nqk_softmax_quant on rows of
    225 .. 1856 (with its row sums) and EPI_PV at K = Tp, each fed the reference's own input of that
    stage: the body of test_gpu_fused_reference.test_three_launch_pieces_equal_the_reference.
    nqk_qgemm_fused has no entry check that refuses any of these parameter sets (it leaves the int32
    zero-point algebra on its own where the bound fails), so every stage runs on every case."""
    check_three_launch_pieces(case)


@pytest.mark.parametrize("q_rows", [1, 16, 17, 256])
def test_long_attention_query_row_prefix_equals_the_reference(q_rows):
    """q_rows = 1, one whole query block, one row into the second, and every row but the one of the
    last block: the rows below q_rows equal the reference, no other byte of ctx is written."""
    T = 257
    d = F.attn_case(F.AttnCase(T, "std", "unit"))
    got = _long(d, T, 8, q_rows=q_rows)
    _equal(got[:, :q_rows], d["ctx"][:, :q_rows], q_rows)
    assert (got[:, q_rows:] == SENTINEL).all(), "a row past the prefix was written"


def test_long_attention_padded_output_rows():
    """ld_out = heads * 64 + 64: the 64 pad columns of every row stay as they were."""
    T = 225
    d = F.attn_case(F.AttnCase(T, "std", "unit"))
    got = _long(d, T, 8, ld_out=H * DH + 64)
    _equal(np.ascontiguousarray(got[:, :, :H * DH]), d["ctx"], T)
    assert (got[:, :, H * DH:] == SENTINEL).all(), "a pad column was written"


@pytest.mark.parametrize("xcds", ["1", "3", "4", "6"])
def test_long_attention_tile_order_for_any_xcd_count(xcds, monkeypatch):
    """6 * 15 = 90 workgroups: no multiple of the device's 8 XCDs nor of 4 (xcd_remap's uneven
    bands), 15 | 30 per band at 6 | 3 (a head's blocks split over two bands at 6).  xcd_count reads
    NQK_XCDS on every call; every tile must be computed once and stored where it belongs (a tile left
    out keeps the sentinel; the six heads' rows differ in kind, so a swapped tile shows)."""
    monkeypatch.setenv("NQK_XCDS", xcds)
    T = 225
    d = F.attn_case(F.AttnCase(T, "std", "unit"))
    _equal(_long(d, T, 8), d["ctx"], T)
