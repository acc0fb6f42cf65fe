"""GPU parity of the float operator layer, one operator at a time: every case calls
numpy_quant.model.onnx_operator_implementation on device tensors and compares the result with
the oracle's per-op NumPy restatement (oracle.nq_oracle._float_op, pinned to the reference's
fixtures by tests/test_oracle.py) or with the plain NumPy expression, on the same host arrays.
Float results are compared as int32 bit patterns, so the sign of zero counts; the one relaxation
is that any NaN equals any NaN at the same position.  Shapes and result kinds (F / I / Q) must
match too.  The inputs and their conditions are tests/_op_cases.py (asserted without a GPU by
tests/test_op_cases_ref.py).

Tanh is the one float op that is not bit-pinned (the device library's tanhf against NumPy's own
implementation): it is held to TANH_BOUND_ULP against a float64 tanh, see test_tanh."""
import numpy as np
import pytest

import _op_cases as C
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev(t):
    from numpy_quant.tensor import FTensor, ITensor, QTensor
    if t[0] == "F":
        return FTensor(t[1])
    if t[0] == "I":
        return ITensor(np.array(t[1]))
    return QTensor(np.array(t[1]), t[2], t[3], t[4])


def run(op, ins, attrs):
    from numpy_quant.model import onnx_operator_implementation
    return onnx_operator_implementation(op, [_dev(t) for t in ins], dict(attrs))


def same_bits(got, ref, what=""):
    """float32 arrays equal bit for bit, any NaN matching any NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == F32 and ref.dtype == F32, (what, got.dtype, ref.dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    g = np.ascontiguousarray(got).reshape(-1)
    r = np.ascontiguousarray(ref).reshape(-1)
    bad = (g.view(np.int32) != r.view(np.int32)) & ~(np.isnan(g) & np.isnan(r))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {k}: "
                             f"{g[k]!r} ({g.view(np.uint32)[k]:#010x}) != {r[k]!r} ({r.view(np.uint32)[k]:#010x})")


def same_tensor(got, ref, what=""):
    """A device tensor against the oracle's tagged tuple: kind, shape, values (and qparams)."""
    kind = {"FTensor": "F", "ITensor": "I", "QTensor": "Q"}[type(got).__name__]
    assert kind == ref[0], (what, kind, ref[0])
    if kind == "F":
        return same_bits(got.data, ref[1], what)
    data = got.data
    assert data.dtype == np.int64 and np.asarray(ref[1]).dtype == np.int64, what
    assert data.shape == np.asarray(ref[1]).shape, (what, data.shape, np.asarray(ref[1]).shape)
    assert np.array_equal(data, ref[1]), what
    if kind == "Q":
        assert (got.bit_width, got.scale, got.zero_point) == tuple(ref[2:5]), what


def check(op, ins, attrs, what=""):
    with np.errstate(all="ignore"):
        ref = O._float_op(op, ins, attrs)
    out = run(op, ins, attrs)
    assert len(out) == len(ref)
    for g, r in zip(out, ref):
        same_tensor(g, r, what or op)


def _ident(shape, axis):
    return "x".join(map(str, shape)) + f"-ax{axis}"


# ----------------------------------------------------------------------------- (a) reductions
REDUCE = [(op, s, a) for s, a in C.reduce_cases() for op in C.REDUCE_OPS if C.applies(op, s)]


@pytest.mark.parametrize("op,shape,axis", REDUCE, ids=[f"{op}-{_ident(s, a)}" for op, s, a in REDUCE])
def test_reduction(op, shape, axis):
    """ReduceMean, Softmax and LayerNormalization over an inner axis (one term at a time, as NumPy
    adds an axis that has elements after it), over an axis followed by extents of 1 only and over
    the last axis (pairwise), each axis spelled both ways."""
    name, ins, attrs, ref = C.reduce_case(op, shape, axis)
    out = run(name, ins, attrs)
    assert len(out) == 1
    same_tensor(out[0], ref[0], f"{name} {shape} axis {axis}")


@pytest.mark.parametrize("op", C.REDUCE_OPS)
def test_last_axis_beyond_the_plan(op):
    """An innermost axis longer than the pairwise plan covers is refused on the host, by name."""
    x = np.zeros((2, C.TOO_LONG), F32)
    p = np.ones(C.TOO_LONG, F32)
    name, ins, attrs = C.op_inputs(op, x, p, p, -1)
    with pytest.raises((ValueError, RuntimeError), match="8192"):
        run(name, ins, attrs)


# ----------------------------------------------------------------------------- (b) special rows
@pytest.mark.parametrize("cols", C.SPECIAL_COLS)
@pytest.mark.parametrize("op", C.REDUCE_OPS)
def test_special_rows(op, cols):
    """Rows of -0.0 (NumPy's sum starts from +0), a constant, an overflowing square, subnormals,
    NaN, infinities and the masked-attention pattern."""
    name, ins, attrs, ref = C.special_case(op, cols)
    out = run(name, ins, attrs)
    for r in range(8):  # row by row, for a readable failure
        same_bits(out[0].data[r], ref[0][1][r], f"{name} cols {cols} row {r}")
    same_tensor(out[0], ref[0], f"{name} cols {cols}")


# ----------------------------------------------------------------------------- (c) unary
@pytest.mark.parametrize("op", ["Erf", "Relu", "Sigmoid"])
def test_unary_op(op):
    x = C.unary_input()
    out = run(op, [O.F(x)], {})
    assert len(out) == 1 and type(out[0]).__name__ == "FTensor"
    same_bits(out[0].data, C.unary_ref(op, x), op)


@pytest.mark.parametrize("name", ["sqrt", "inv", "exp", "neg"])
def test_unary_method(name):
    from numpy_quant.tensor import FTensor
    x = C.unary_input()
    t = FTensor(x)
    out = -t if name == "neg" else getattr(t, name)()
    same_bits(out.data, C.unary_ref(name, x), name)


def test_tanh():
    """The device's tanhf against tanh in float64: within one ulp of what NumPy's own float32
    tanh reaches (1.36 ulp, so 2.36), and exactly NumPy's result at +-0, +-inf, NaN and where
    tanh has saturated to +-1.  Measured on the MI355X: at most 0.854 ulp on this vector (at
    x = -0.68559223); the figure is printed below and kept in DESIGN.md (parity)."""
    x = C.unary_input()
    out = run("Tanh", [O.F(x)], {})
    assert len(out) == 1 and type(out[0]).__name__ == "FTensor"
    got = out[0].data
    assert got.shape == x.shape and got.dtype == F32
    err, mask = C.tanh_ulp_error(x, got)
    worst = int(np.argmax(np.where(mask, err, -1)))
    print(f"device tanhf: max {err[mask].max():.3f} ulp at x = {x[worst]!r}")
    assert err[mask].max() <= C.TANH_BOUND_ULP
    exact = ~mask | (x == 0) | (np.abs(x) >= C.TANH_SATURATED)
    same_bits(got[exact], np.tanh(x[exact]), "Tanh special values")
    assert np.isnan(got[np.isnan(x)]).all() and np.isnan(x).any()


# ----------------------------------------------------------------------------- (d) binary
BIN_OPS = ["Add", "Sub", "Mul", "Div"]


def _binary(op, a, b):
    if op == "Sub":  # as the reference spells it: a + (-b)
        from numpy_quant.tensor import FTensor
        return FTensor(a) + (-FTensor(b))
    out = run(op, [O.F(a), O.F(b)], {})
    assert len(out) == 1
    return out[0]


@pytest.mark.parametrize("pair", [0, 1], ids=["all-pairs", "reversed"])
@pytest.mark.parametrize("op", BIN_OPS)
def test_binary_special_values(op, pair):
    """0/0, inf - inf, x/0, 0 * inf, subnormal and overflowing results: all IEEE, bit for bit."""
    a, b = C.special_pairs()[pair]
    same_bits(_binary(op, a, b).data, C.binary_ref(op, a, b), op)


@pytest.mark.parametrize("sa,sb", C.BROADCASTS, ids=[f"{a}-{b}".replace(" ", "") for a, b in C.BROADCASTS])
@pytest.mark.parametrize("op", BIN_OPS)
def test_binary_broadcast(op, sa, sb):
    a, b = C.broadcast_pair(sa, sb)
    same_bits(_binary(op, a, b).data, C.binary_ref(op, a, b), f"{op} {sa} {sb}")


@pytest.mark.parametrize("s", C.SCALARS)
def test_add_python_float(s):
    from numpy_quant.tensor import FTensor
    for x in (C.unary_input(), C.broadcast_pair(*C.BROADCASTS[0])[0]):
        with np.errstate(all="ignore"):
            ref = x + s  # a Python float joins a float32 array as float32
        same_bits((FTensor(x) + s).data, ref, f"x + {s}")
        same_bits((s + FTensor(x)).data, ref, f"{s} + x")


# ----------------------------------------------------------------------------- (e) structural
@pytest.mark.parametrize("idx,axis", C.GATHER, ids=[f"{i.shape}-ax{a}".replace(" ", "") for i, a in C.GATHER])
def test_gather(idx, axis):
    x = C.struct_array((5, 6, 7))
    check("Gather", [O.F(x), O.I(idx.astype(np.int64))], {"axis": axis})
    same_bits(run("Gather", [O.F(x), O.I(idx.astype(np.int64))], {"axis": axis})[0].data, np.take(x, idx, axis))


@pytest.mark.parametrize("idx,axis", C.GATHER_BAD, ids=[f"{i.shape}-ax{a}".replace(" ", "") for i, a in C.GATHER_BAD])
def test_gather_out_of_range(idx, axis):
    with pytest.raises(IndexError):
        run("Gather", [O.F(C.struct_array((5, 6, 7))), O.I(idx.astype(np.int64))], {"axis": axis})


def test_gather_itensor():
    shape = np.array([2, 197, 768], np.int64)
    check("Gather", [O.I(shape), O.I(np.array(1, np.int64))], {"axis": 0})
    check("Gather", [O.I(shape), O.I(np.array([-1, 0], np.int64))], {"axis": 0})


@pytest.mark.parametrize("spec", C.SLICE, ids=[f"{s[0]}-{s[2]}".replace(" ", "") for s in C.SLICE])
def test_slice(spec):
    x = C.struct_array((5, 6, 7))
    ins = [O.F(x)] + [O.I(np.array(v, np.int64)) for v in spec]
    check("Slice", ins, {})
    same_bits(run("Slice", ins, {})[0].data, x[C.slice_index(spec, 3)])


@pytest.mark.parametrize("shapes,axis", C.CONCAT, ids=[f"ax{a}" for _, a in C.CONCAT])
def test_concat(shapes, axis):
    parts = [C.struct_array(s, f"concat{k}") for k, s in enumerate(shapes)]
    check("Concat", [O.F(p) for p in parts], {"axis": axis})
    check("Concat", [O.I(np.arange(3)), O.I(np.array([-1])), O.I(np.array([7, 8]))], {"axis": 0})


@pytest.mark.parametrize("shape,target", C.EXPAND, ids=[f"{s}-{t}".replace(" ", "") for s, t in C.EXPAND])
def test_expand(shape, target):
    check("Expand", [O.F(C.struct_array(shape)), O.I(np.array(target, np.int64))], {})


@pytest.mark.parametrize("sc,sa,sb,kind", C.WHERE, ids=[f"{c}-{a}-{b}-{k}".replace(" ", "") for c, a, b, k in C.WHERE])
def test_where(sc, sa, sb, kind):
    rng = np.random.default_rng(len(sc) + 10 * len(sa))
    cond = {"mixed": rng.integers(0, 2, size=sc), "true": np.ones(sc), "false": np.zeros(sc)}[kind].astype(np.int64)
    a, b = C.struct_array(sa, "where-a"), C.struct_array(sb, "where-b")
    assert kind != "mixed" or (cond.any() and not cond.all())
    check("Where", [O.I(cond), O.F(a), O.F(b)], {})
    same_bits(run("Where", [O.I(cond), O.F(a), O.F(b)], {})[0].data, np.where(cond, a, b))
    check("Where", [O.I(cond), O.I(np.full(sa, 3)), O.I(np.full(sb, -4))], {})


def test_where_too_many_dimensions():
    """More than 6 dimensions that cannot be merged: the same ValueError as the binary ops."""
    cond = np.ones((2, 1, 2, 1, 2, 1, 2), np.int64)
    a = np.zeros((1, 2, 1, 2, 1, 2, 1), F32)
    for call in (lambda: run("Where", [O.I(cond), O.F(a), O.F(np.zeros((), F32))], {}),
                 lambda: run("Add", [O.F(cond.astype(F32)), O.F(a)], {})):
        with pytest.raises(ValueError, match="more than 6 non-mergeable dimensions"):
            call()


def test_equal_shape_identity():
    a = np.array([1, 197, -1, 768], np.int64)
    check("Equal", [O.I(a), O.I(np.array([1, 196, -1, 768], np.int64))], {})
    check("Equal", [O.I(a), O.I(np.array(-1, np.int64))], {})
    x = C.struct_array((3, 1, 5))
    check("Shape", [O.F(x)], {})
    check("Shape", [O.I(a)], {})
    check("Identity", [O.F(x)], {})
    from numpy_quant.model import onnx_operator_implementation as impl
    t = _dev(O.F(x))
    assert impl("Identity", [t], {})[0].dev.ptr != t.dev.ptr  # a copy, not an alias


def test_reshape_transpose_float():
    x = C.struct_array((2, 3, 4))
    check("Reshape", [O.F(x), O.I(np.array([4, -1], np.int64))], {})
    check("Reshape", [O.F(x), O.I(np.array([-1], np.int64))], {})
    empty = np.zeros((2, 0, 3), F32)
    check("Reshape", [O.F(empty), O.I(np.array([0, 6], np.int64))], {})  # NumPy's 0 is a literal 0
    with pytest.raises(ValueError):
        run("Reshape", [O.F(x), O.I(np.array([0, 24], np.int64))], {})
    check("Reshape", [O.I(np.arange(6)), O.I(np.array([2, -1], np.int64))], {})
    check("Transpose", [O.F(x)], {"perm": None})  # the default: every axis reversed
    check("Transpose", [O.F(x)], {"perm": [1, 2, 0]})
    check("Transpose", [O.F(C.struct_array((3, 4, 5, 2)))], {"perm": None})


def test_unsqueeze_first_row():
    """model.py:203-206 returns the tensor itself where a list is expected; the executor's zip then
    takes its first row.  Kept bug-compatible."""
    from numpy_quant.tensor import ITensor
    for data, axes in ((np.array([[3, 4], [5, 6]], np.int64), [0]), (np.array([7, 8, 9], np.int64), [1]),
                       (np.array([7, 8, 9], np.int64), [0])):
        ins = [O.I(data), O.I(np.array(axes, np.int64))]
        ref = O._float_op("Unsqueeze", ins, {})
        out = run("Unsqueeze", ins, {})
        first = [t for _, t in zip(ref, out)]
        assert len(first) == 1 and isinstance(first[0], ITensor)
        same_tensor(first[0], ref[0], f"Unsqueeze {axes}")


def test_constant_of_shape():
    for value in (np.array([2.5], F32), np.array([-0.0], F32), np.array([7], np.int64)):
        for shape in ([2, 3], [4], [0, 3], [1, 1, 5]):
            check("ConstantOfShape", [O.I(np.array(shape, np.int64))], {"value": value})
    check("Constant", [], {"value": C.struct_array((2, 2))})
    check("Constant", [], {"value": np.array([1, -1], np.int64)})


@pytest.mark.parametrize("bw", C.QBITS)
def test_qtensor_transpose_reshape(bw):
    """Transpose and Reshape of quantized tensors: storage of 1, 2, 4 and 8 bytes per element."""
    from numpy_quant import kernels as K
    q = C.qtensor_data(bw)
    t = O.Q(q, bw, F32(0.0625), np.array(-3, np.int64))
    assert _dev(t).dev.dtype.itemsize == {8: 1, 12: 2, 32: 4, 40: 8}[bw] == K.storage_dtype(bw).itemsize
    for perm in ([2, 0, 1], [1, 0, 2], [0, 2, 1]):
        check("Transpose", [t], {"perm": perm}, f"Transpose bw {bw} {perm}")
    check("Reshape", [t, O.I(np.array([-1, 7], np.int64))], {}, f"Reshape bw {bw}")
    from numpy_quant.model import onnx_operator_implementation as impl
    from numpy_quant.tensor import ITensor
    tr = impl("Transpose", [_dev(t)], {"perm": [2, 1, 0]})[0]  # a reshape of the permuted copy
    out = impl("Reshape", [tr, ITensor(np.array([5, -1], np.int64))], {})
    same_tensor(out[0], O.Q(q.transpose(2, 1, 0).reshape(5, -1), bw, F32(0.0625), np.array(-3, np.int64)))
