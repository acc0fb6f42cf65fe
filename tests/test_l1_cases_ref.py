"""The conditions on the inputs of tests/test_gpu_l1_kernels.py, asserted on the NumPy reference
alone (no GPU): every table of tests/_l1_cases.py reaches the edge it claims — exact rounding ties
that tell half-even from half-away, outputs on both clip bounds, accumulators float64 cannot hold,
zero-point terms that change when the wrong batch is read, products an int32 accumulator cannot
hold, sizes past each kernel's grid.  They are conditions, not measurements: the "wrong" variants
here are variants of the reference, never of the product."""
import platform

import numpy as np
import pytest

import _l1_cases as C
from oracle import nq_oracle as O


# ----------------------------------------------------------------------------- group 1
def test_nan_is_int64_min_on_this_host():
    """The kernels give INT64_MIN for NaN, NumPy's float -> int64 on x86 (cvttsd2si)."""
    if platform.machine().lower() not in ("x86_64", "amd64", "i686", "i386"):
        pytest.skip(f"NaN -> int64 is pinned to x86's conversion; this host is {platform.machine()}: "
                    "the NaN element is checked against INT64_MIN on the GPU only")
    with np.errstate(all="ignore"):
        for bw, (s, zp) in ((8, (0.5, None)), (8, (0.5, 3)), (32, (1, None)), (32, (0.031, 1 << 20))):
            q = O.quantize(np.array([np.nan], C.F32), bw, C.F32(s), C.zp_arr(zp))
            assert q[0] == C.INT64_MIN, (bw, s, zp, q)


@pytest.mark.parametrize("bw", C.BIT_WIDTHS)
def test_quantize_tables(bw):
    lo, hi = O.qrange(bw)
    for scale, zp in C.QPARAMS:
        x = C.quant_input(bw, scale, zp)
        ref = C.quant_ref(bw, scale, zp)
        normals, ties, ladder, special = C.quant_parts(bw, scale, zp)
        assert x.dtype == C.F32 and x.size == normals.size + ties.size + ladder.size + special.size
        assert np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
        # the restated first step agrees with the oracle: clip, then round half-even
        u = C.preclip(x, scale, zp)
        ok = ~np.isnan(x)
        b_lo, b_hi = (u.dtype.type(lo), u.dtype.type(hi))
        with np.errstate(all="ignore"):
            again = np.rint(np.minimum(np.maximum(u, b_lo), b_hi)).astype(np.int64)
        np.testing.assert_array_equal(again[ok], ref[ok])
        assert (ref[~ok] == C.INT64_MIN).all()
        # clips: the ladder holds unclipped, lower-clipped and upper-clipped values
        ul = C.preclip(ladder, scale, zp)
        assert (ul < b_lo).any() and (ul > b_hi).any() and ((ul >= b_lo) & (ul <= b_hi)).any(), (bw, scale, zp)
        rl = ref[normals.size + ties.size:][:ladder.size]
        assert (rl == int(lo)).any() and (rl == int(np.rint(b_hi))).any(), (bw, scale, zp)
        # ties: at least 100 exact k + 0.5, on which half-even and half-away differ in 40 %
        if scale in C.POW2_SCALES:
            ut = C.preclip(ties, scale, zp).astype(np.float64)
            tie = ut - np.floor(ut) == 0.5
            assert tie.sum() >= 100, (bw, scale, zp, int(tie.sum()))
            differ = np.rint(ut[tie]) != C.half_away(ut[tie])
            assert differ.mean() >= 0.4, (bw, scale, zp, differ.mean())
            if bw >= 12:  # wide enough that the clip leaves the ties alone: the outputs differ too
                rt = ref[normals.size:][:ties.size]
                away = np.clip(C.half_away(ut), lo, hi).astype(np.int64)
                assert (rt[tie] != away[tie]).mean() >= 0.4, (bw, scale, zp)


def test_bit_width_32_saturates_at_2_pow_31():
    """Defect 2: without a zero point the clip is in float32, float32(2^31 - 1) = 2^31, and the
    reference's result does not fit int32."""
    for scale, zp in C.QPARAMS:
        ref = C.quant_ref(32, scale, zp)
        ok = ~np.isnan(C.quant_input(32, scale, zp))
        assert (ref[ok].max() == 2 ** 31) == (zp is None), (scale, zp)
        assert ref[ok].min() == -2 ** 31
    for bw in C.BIT_WIDTHS[:-1]:
        for scale, zp in C.QPARAMS:
            ref = C.quant_ref(bw, scale, zp)[~np.isnan(C.quant_input(bw, scale, zp))]
            info = np.iinfo(C.storage(bw))
            assert info.min <= ref.min() and ref.max() <= info.max, (bw, scale, zp)


def test_flat_and_row_sizes():
    assert max(C.FLAT_N) > C.FLAT_GRID and sorted(C.FLAT_N)[-2] < C.FLAT_GRID
    assert {n % 4 for n in C.FLAT_N} == {0, 1, 2, 3}
    assert C.UNALIGNED_N % 4 == 3
    bw, s, zp = C.FLAT_QP
    x = C.flat_input(1023)
    q = C.quantize_ref(x, bw, s, zp)
    u = C.preclip(x, s, zp)
    assert (u - np.floor(u) == 0.5).mean() > 0.2 and (q == -128).any() and (q == 127).any()
    assert max(r for r, _ in C.ROW_SHAPES) > C.ROW_GRID
    assert {n % 64 for _, n in C.ROW_SHAPES} >= {1, 63, 0, 5} and any(n > 64 * 64 for _, n in C.ROW_SHAPES)
    for bw, s, zp in C.ROW_QP:
        q = C.quantize_ref(C.row_input(300, 197), bw, s, zp)
        lo, hi = O.qrange(bw)
        f = C.clip_fractions(q, bw)
        assert f[2] > 0.5 and (bw == 12 or (f[0] > 0 and f[1] > 0)), (bw, s, zp, f)


# ----------------------------------------------------------------------------- group 2
@pytest.mark.parametrize("form", C.ZP_FORMS)
def test_big_accumulators_round_in_float64(form):
    acc = C.big_acc()
    v = C.centred(acc, C.zp_form(form, C.BIG_SHAPE))
    inexact, half = C.f64_inexact(v)
    assert inexact.sum() >= 8 and (inexact & half).sum() >= 1, (form, int(inexact.sum()), int(half.sum()))
    if form == "none":
        assert float(2 ** 53 + 1) == 2.0 ** 53 and float(2 ** 53 + 3) == 2.0 ** 53 + 4
        assert float(-2 ** 62 - 2 ** 9 - 1) == -2.0 ** 62 - 2.0 ** 10
        flat = [int(t) for t in acc.reshape(-1)]
        assert {2 ** 53 + 1, 2 ** 53 + 3, -2 ** 62 - 2 ** 9 - 1, 2 ** 24, -2 ** 31, 2 ** 31} <= set(flat)


@pytest.mark.parametrize("bw", C.TIE_BW)
def test_requantize_ties_and_clips(bw):
    acc = C.tie_acc(bw)
    lo, hi = O.qrange(bw)
    d = O.dequantize(acc, C.TIE_ARR_SCALE, None)
    v = (C.F32(1) / C.TIE_RES_SCALE) * d
    tie = (v.astype(np.float64) - np.floor(v.astype(np.float64))) == 0.5
    assert tie.sum() >= 100
    assert (np.rint(v[tie]) != C.half_away(v[tie])).mean() >= 0.4
    for rz in C.TIE_RES_ZP:
        q = O.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, C.zp_arr(rz), bw)
        top = int(np.rint(C.F32(hi))) if rz is None else int(hi)
        assert (q == int(lo)).any() and (q == top).any() and ((q > lo) & (q < hi)).any(), (bw, rz)


def test_requantize_reaches_2_pow_31():
    acc = C.sat32_acc()
    q = O.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, None, 32)
    assert (q == 2 ** 31).sum() >= 3 and (q == -2 ** 31).sum() >= 3 and (np.abs(q) < 2 ** 31).any()
    q = O.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, C.zp_arr(-3), 32)
    assert q.max() == 2 ** 31 - 1


def test_stride_array_exceeds_the_grid():
    acc, zp = C.stride_acc()
    assert acc.size > C.STRIDE_GRID and zp.shape == (1, acc.shape[1])
    assert 2 ** 20 + 5 in C.RELU_N and 2 ** 20 + 5 > C.STRIDE_GRID
    assert any(s[0] * s[1] > C.ROW_GRID for s in C.ROWSUM_SHAPES)


# ----------------------------------------------------------------------------- group 3
def test_routes():
    """Which kernel a shape takes at int8 storage: M * N * K against kernels.MFMA_MIN_WORK."""
    work = {name: sa[-2] * sa[-1] * sb[-1] for name, sa, sb, _ in C.MM_SHAPES}
    assert work["generic"] < C.MFMA_MIN_WORK and work["materialised-generic"] < C.MFMA_MIN_WORK
    for name in C.MM_NAMES:
        if "generic" not in name:
            assert work[name] >= C.MFMA_MIN_WORK, name
    assert C.mm_shape("mfma-padded-k")[1][-1] % 16 and C.mm_shape("mfma-tile-edge")[1][-2] == 129
    sa, sb = C.mm_shape("grid-stride")[1:3]
    assert sa[0] * sb[1] > C.STRIDE_GRID


@pytest.mark.parametrize("bw", C.MM_BW)
@pytest.mark.parametrize("name", C.MM_NAMES)
def test_requantize_clips_on_both_sides(name, bw):
    lo, hi = (int(v) for v in O.qrange(bw))
    for zpair in C.ZP_PAIRS:
        case = C.mm_case(name, bw, zpair)
        for t, extent in ((case["a"], (lo, hi)), (case["b"], (lo, hi))):
            assert t.min() == extent[0] and t.max() == extent[1]
        # a product of one sign can reach one bound only: (a + 138) > 0 and (b - 11) < 0 for every
        # 4-bit a and b, and no other combination
        assert case["one_sided"] == (bw == 4 and zpair == (-138, 11)), (name, bw, zpair)
        for (kind, rz), (rs, q) in case["requant"].items():
            f_lo, f_hi, f_in = C.clip_fractions(q, bw)
            what = (name, bw, zpair, kind, rz, float(rs), f_lo, f_hi, f_in)
            assert f_in >= 0.5, what
            if case["one_sided"]:
                assert max(f_lo, f_hi) >= 0.1, what
            else:
                assert f_lo >= 0.1 and f_hi >= 0.1, what


@pytest.mark.parametrize("bw", C.MM_BW)
@pytest.mark.parametrize("name", [n for n, sa, sb, _ in C.MM_SHAPES if len(sa) > 2 or len(sb) > 2])
def test_wrong_batch_changes_every_slice(name, bw):
    """The term with A's row sums, and separately B's column sums, rolled by one along each batched
    axis of extent > 1: the requantized reference changes in every output batch slice.  Asserted
    for every zero-point pair that holds the rolled sums, but the one whose products are of one
    sign (4 bits, (-138, 11)): its outputs lie within 5 % of their mean, so one output step is some
    3500 accumulator units and the rolled row sums (times 11) move less than that; there the row
    sums are pinned by the pair (None, 11), the column sums by (-138, None), and the term itself,
    which the GPU test compares directly, differs in every slice."""
    rolled = 0
    for zpair in C.ZP_PAIRS[1:]:
        case = C.mm_case(name, bw, zpair)
        a, b, acc, s = case["a"], case["b"], case["acc"], case["s"]
        rs, ref = case["requant"]["none", None]
        nb = int(np.prod(acc.shape[:-2]))
        full = np.broadcast_to(case["term"], acc.shape)
        for which, t, present in (("row", a, zpair[1] is not None), ("col", b, zpair[0] is not None)):
            for axis in range(t.ndim - 2):
                if t.shape[axis] < 2 or not present:
                    continue
                term = C.zp_term(a, b, *zpair, **{"roll_" + which: axis})
                assert (np.broadcast_to(term, acc.shape) != full).reshape(nb, -1).any(axis=1).all()
                if not case["one_sided"]:
                    q = O.requantize(acc, s, term, rs, None, bw)
                    changed = (q != ref).reshape(nb, -1).any(axis=1)
                    assert changed.all(), (name, bw, zpair, which, axis, changed)
                rolled += 1
    assert rolled >= 2


def test_mixed_sums_pass_2_pow_53():
    for i, (ta, _, tb, _) in enumerate(C.MIXED):
        a, b, ref = C.mixed_case(i)
        assert a.dtype == ta and b.dtype == tb and ref.shape == (37, 29)
        np.testing.assert_array_equal(ref, np.matmul(a.astype(np.int64), b.astype(np.int64)))
        if np.dtype(ta).itemsize + np.dtype(tb).itemsize >= 9:
            assert np.abs(ref).max() > 2 ** 53


# ----------------------------------------------------------------------------- group 4
@pytest.mark.parametrize("k", C.ACC_K)
def test_int32_accumulator_bound(k):
    """Defect 1: K = 131072 products of -128 * -128 are 2^31; up to K = 131071 int32 is exact."""
    for zpair in C.ACC_ZP:
        a, b, acc, s, term = C.acc_case(k, zpair)
        assert 4 * k >= C.MFMA_MIN_WORK
        wraps = (acc != C.wrap32(acc)).sum()
        if k == 131056:
            assert k % 16 == 0 and k + 16 > 131071 and wraps == 0
        elif k == 131072:
            assert acc[0, 0] == 2 ** 31 and wraps == 1
        else:
            assert (k % 16 != 0) == (k == 140001) and wraps >= 2
        assert (term is None) == (zpair == (None, None))


# ----------------------------------------------------------------------------- group 5
@pytest.mark.parametrize("dt", C.RELU_DTYPES)
def test_relu_tables(dt):
    info = np.iinfo(dt)
    for zp, outside in C.relu_zero_points(dt):
        assert outside == (not info.min <= zp <= info.max)
        q, ref = C.relu_case(dt, 255, zp)
        assert q.dtype == dt and ref.dtype == np.int64
        assert ref.min() >= zp and (q == info.min).any() and (q == info.max).any()
        if not outside:
            assert (q == zp).any()
        if info.min < zp < info.max:
            assert (q == zp - 1).any() and (q == zp + 1).any() and (ref != q).any() and (ref == q).any()
        if zp > info.max:
            assert (ref == zp).all()
        if zp <= info.min:
            np.testing.assert_array_equal(ref, q.astype(np.int64))


def test_rowsum_tables():
    assert {s[2] for s in C.ROWSUM_SHAPES} >= {1, 63, 64, 65, 200}
    assert any(s[3] > s[2] for s in C.ROWSUM_SHAPES) and any(s[4] > s[1] * s[3] for s in C.ROWSUM_SHAPES)
    assert any(s[0] * s[1] == 16384 + 3 for s in C.ROWSUM_SHAPES)
    for dt in C.RELU_DTYPES:
        buf, ref = C.rowsum_case(dt, (2, 3, 64, 70, 250))
        assert buf.dtype == dt and ref.shape == (6,)
        assert ref[4] == buf[250 + 70:250 + 70 + 64].astype(np.int64).sum()
