"""The input conditions of tests/test_gpu_ops.py, asserted on the NumPy reference alone (no GPU):
which summation order this NumPy takes for each shape and axis, that the two orders can be told
apart on the chosen data, and where NaN and inf may appear.  If a future NumPy changes its
reduction order, the first two tests fail and say so."""
import numpy as np
import pytest

import _op_cases as C

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.int32)


def _ident(shape, axis):
    return "x".join(map(str, shape)) + f"-ax{axis}"


TABLE = [(s, a, "sequential") for s, a in C.SEQUENTIAL] + [(s, a, "pairwise") for s, a in C.PAIRWISE]


@pytest.mark.parametrize("shape,axis,order", TABLE, ids=[_ident(s, a) + "-" + o for s, a, o in TABLE])
def test_numpy_summation_order(shape, axis, order):
    """x.sum(axis) of a contiguous float32 array: one term at a time in index order when elements
    follow the axis, pairwise when only extents of 1 do."""
    x = C.reduce_case("ReduceMean1", shape, axis)[1][0][1]
    assert x.flags.c_contiguous and x.dtype == F32
    got = _bits(x.sum(axis=axis, keepdims=True))
    seq, pw = _bits(C.sequential_sum(x, axis)), _bits(C.pairwise_sum(x, axis))
    hint = f"NumPy {np.__version__} no longer sums {shape} over axis {axis} in {order} order"
    assert np.array_equal(got, seq if order == "sequential" else pw), hint
    assert not np.array_equal(got, pw if order == "sequential" else seq), "the data cannot tell the orders apart"


OP_TABLE = [(op, s, a, o) for s, a, o in TABLE for op in C.REDUCE_OPS if C.applies(op, s)]


@pytest.mark.parametrize("op,shape,axis,order", OP_TABLE, ids=[f"{op}-{_ident(s, a)}-{o}" for op, s, a, o in OP_TABLE])
def test_reference_follows_the_order(op, shape, axis, order):
    """The reference of every table case is the op's chain with that order of summation, and a
    sequential case differs from the move-last pairwise form in at least half of its outputs."""
    name, ins, attrs, ref = C.reduce_case(op, shape, axis)
    assert ref[0][1].dtype == F32
    with np.errstate(all="ignore"):
        seq = C.with_sum(name, ins, attrs, C.sequential_sum)
        pw = C.with_sum(name, ins, attrs, C.pairwise_sum)
    same, other = (seq, pw) if order == "sequential" else (pw, seq)
    assert same.shape == ref[0][1].shape
    assert np.array_equal(_bits(ref[0][1]), _bits(same))
    differ = np.mean(_bits(ref[0][1]) != _bits(other))
    print(f"{name} {shape} axis {axis}: {100 * differ:.0f} % of the outputs differ from the other order")
    # a mean and a Softmax differ in at least half of the outputs of a sequential case;
    # LayerNormalization takes the same mean, but a last-bit change of it reaches only the outputs
    # whose later roundings do not absorb it.  (That a pairwise case differs from the sequential
    # order is test_numpy_summation_order's.)
    if order == "sequential":
        assert differ >= 0.5 if name != "LayerNormalization" else differ > 0


def test_both_spellings_share_the_data():
    for shape, axis in C.SEQUENTIAL + C.PAIRWISE:
        for op in C.REDUCE_OPS:
            if C.applies(op, shape):
                a, b = C.reduce_case(op, shape, axis), C.reduce_case(op, shape, axis - len(shape))
                assert b[2]["axis"] < 0 <= a[2]["axis"]
                assert np.array_equal(_bits(a[3][0][1]), _bits(b[3][0][1]))


def test_reduction_references_are_finite():
    for shape, axis in C.reduce_cases():
        for op in C.REDUCE_OPS:
            if C.applies(op, shape):
                name, ins, attrs, ref = C.reduce_case(op, shape, axis)
                assert all(np.isfinite(t[1]).all() for t in ins), (op, shape)
                assert np.isfinite(ref[0][1]).all(), (op, shape)
                assert ref[0][1].size < 2_000_000 and ins[0][1].size < 2_000_000


def test_last_axis_cases_cover_the_plan():
    """Every branch of the pairwise plan: n < 8, a block with and without a tail, the split above
    128, trees of 2, 3 (unbalanced), 8 and 64 leaves, and the limit itself."""
    def leaves(n):
        if n <= 128:
            return [n]
        h = n // 2 - (n // 2) % 8
        return leaves(h) + leaves(n - h)
    plans = {c: leaves(c) for c in C.LAST_COLS}
    assert any(c < 8 for c in plans) and 8 in plans and any(8 < c <= 128 and c % 8 for c in plans)
    assert len(plans[128]) == 1 and len(plans[129]) == 2
    assert any(len(p) & (len(p) - 1) for p in plans.values()), "no unbalanced tree"
    assert len(plans[8192]) == 64 and max(len(p) for p in plans.values()) == 64
    assert len(leaves(C.TOO_LONG)) > 64
    assert C.MANY_ROWS[0] > 65536 * 4


@pytest.mark.parametrize("cols", C.SPECIAL_COLS)
def test_special_rows(cols):
    """NaN appears exactly in the rows designed for it; everything else is finite but the means of
    the rows that hold an infinity."""
    x = C.special_rows(cols)
    assert np.all(np.signbit(x[C.ROW_NEG_ZERO])) and not x[C.ROW_NEG_ZERO].any()
    sub = x[C.ROW_SUBNORMAL]
    assert np.all((sub > 0) & (sub < np.finfo(F32).tiny))
    assert np.isnan(x[C.ROW_NAN]).sum() == 1 and np.isposinf(x[C.ROW_PINF]).sum() == 1
    masked = x[C.ROW_MASKED]
    assert np.isneginf(masked).any() and np.isfinite(masked).any() and not np.isnan(masked).any()

    nan_rows = {  # rows 5-7 of the list for Softmax; a mean keeps an infinity, a variance does not
        "Softmax": [C.ROW_NAN, C.ROW_ALL_NINF, C.ROW_PINF],
        "ReduceMean1": [C.ROW_NAN],
        "LayerNormalization": [C.ROW_NAN, C.ROW_ALL_NINF, C.ROW_PINF, C.ROW_MASKED]}
    for op, rows in nan_rows.items():
        ref = C.special_case(op, cols)[3][0][1]
        expect = np.zeros(ref.shape, bool)
        expect[rows] = True
        assert np.array_equal(np.isnan(ref), expect), op
    sm = C.special_case("Softmax", cols)[3][0][1]
    assert np.isfinite(sm[C.ROW_MASKED]).all() and (sm[C.ROW_MASKED] == 0).sum() == np.isneginf(masked).sum()
    mean = C.special_case("ReduceMean1", cols)[3][0][1]
    assert _bits(mean[C.ROW_NEG_ZERO])[0] == 0, "NumPy's sum starts from +0: the mean of -0.0 is +0.0"
    assert np.isneginf(mean[[C.ROW_ALL_NINF, C.ROW_MASKED]]).all() and np.isposinf(mean[C.ROW_PINF]).all()
    assert np.isfinite(np.delete(mean, [C.ROW_NAN, C.ROW_ALL_NINF, C.ROW_PINF, C.ROW_MASKED], axis=0)).all()
    ln = C.special_case("LayerNormalization", cols)[3][0][1]
    # x - mean is -0 in the all -0.0 row (mean +0.0) and +0 in the constant row: with beta[0] = -0.0
    # the sign reaches the output
    assert _bits(ln[C.ROW_NEG_ZERO])[0] == np.int32(-2 ** 31) and _bits(ln[C.ROW_CONST])[0] == 0
    assert np.isfinite(ln[C.ROW_HUGE]).all()  # variance inf, 1 / std = 0


def test_unary_vector():
    x = C.unary_input()
    assert x.size == C.UNARY_LEN and x.size % 2 == 1
    for v in (0.0, 1e-45, 1e-38, 1.0, 88.7, 104.0, 3.4e38, np.inf):
        for s in (v, -v):
            hit = x[:C.SPECIALS.size] == F32(s)
            assert (hit & (np.signbit(x[:C.SPECIALS.size]) == np.signbit(F32(s)))).any(), s
    assert np.isnan(x[:C.SPECIALS.size]).any()
    # outside the special values and the random bit patterns, every bit-pinned op but sqrt is finite
    plain = x[C.SPECIALS.size:C.SPECIALS.size + 2048]
    for name in ("Erf", "Relu", "Sigmoid", "exp", "neg"):
        assert np.isfinite(C.unary_ref(name, plain)).all(), name
    assert np.isfinite(C.unary_ref("sqrt", np.abs(plain))).all()


def test_numpy_tanh_error():
    """The figure the device's bound is built on, re-measured on this NumPy."""
    x = np.linspace(-10, 10, 2 ** 20, dtype=F32)
    err, mask = C.tanh_ulp_error(x, np.tanh(x))
    print(f"np.tanh float32: max {err[mask].max():.3f} ulp")
    assert err[mask].max() <= C.TANH_NUMPY_ULP
    big = np.array([C.TANH_SATURATED, 12, 88.7, 3.4e38, np.inf], F32)
    assert np.all(np.tanh(big) == 1) and np.all(np.tanh(-big) == -1)
    assert np.all(np.tanh(big.astype(np.float64)).astype(F32) == 1)


def test_binary_cases():
    for sa, sb in C.BROADCASTS:
        a, b = C.broadcast_pair(sa, sb)
        for name in ("Add", "Sub", "Mul", "Div"):
            assert np.isfinite(C.binary_ref(name, a, b)).all(), (name, sa, sb)
        for s in C.SCALARS:
            assert np.isfinite(a + F32(s)).all()
    a, b = C.special_pairs()[0]
    with np.errstate(all="ignore"):
        q, d = a / b, a + (-b)
    assert np.isnan(q).any() and np.isinf(q).any() and np.isnan(d).any()
    assert ((q != 0) & (np.abs(q) < np.finfo(F32).tiny)).any(), "no subnormal quotient"


def test_structural_inputs():
    for bw in C.QBITS:
        q = C.qtensor_data(bw)
        assert q.min() == -(1 << (bw - 1)) and q.max() == (1 << (bw - 1)) - 1
    x = C.struct_array((5, 6, 7))
    assert np.isfinite(x).all()
    empties = [spec for spec in C.SLICE if x[C.slice_index(spec, x.ndim)].size == 0]
    assert empties, "no empty slice"
    for idx, axis in C.GATHER_BAD:
        with pytest.raises(IndexError):
            x.take(idx, axis)
