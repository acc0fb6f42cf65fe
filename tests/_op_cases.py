"""Inputs of tests/test_gpu_ops.py and their NumPy references, built on the host alone so that
the input conditions — which summation order NumPy takes for a shape and axis, where NaN may
appear, that the two orders can be told apart — are asserted on the reference itself
(tests/test_op_cases_ref.py runs them without a GPU).  Tensors are the oracle's tagged tuples
('F' | 'I' | 'Q', array, ...); every builder is seeded by its own arguments and cached: one
reference per case, shared by all tests, never modified."""
import functools
import zlib

import numpy as np

from oracle import nq_oracle as O

F32 = np.float32
EPS = 1e-12  # LayerNormalization epsilon of every case

# ----------------------------------------------------------------------------- (a) reductions
# shape, axis: NumPy adds these axes one term at a time (an axis with elements after it) ...
SEQUENTIAL = [((1000, 5), 0), ((3, 197, 7), 1), ((2, 9, 4), 1), ((2, 3, 50, 6), 2), ((4, 40, 3, 5), 1),
              ((130, 2, 2), 0), ((1, 8193, 2), 1), ((2, 300, 1, 3), 1)]
# ... and these pairwise: only extents of 1 follow the axis, it is effectively the innermost
PAIRWISE = [((300, 1), 0), ((5, 300, 1), 1), ((2, 300, 1, 1), 1)]
# last axis: each decision point of the pairwise plan (n < 8, the 8-accumulator block and its
# tail, the split above 128, unbalanced and balanced trees, the 64-leaf maximum)
LAST_COLS = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 255, 256, 257, 1023, 1025, 4097, 8192]
MANY_ROWS = (65536 * 4 + 3, 2)  # more rows than the row kernels' grid
TOO_LONG = 8193  # one more than the pairwise plan covers
REDUCE_OPS = ("ReduceMean0", "ReduceMean1", "Softmax", "LayerNormalization")


def reduce_cases():
    """[(shape, axis)] of (a): the table with each axis spelled both ways, then the last axis."""
    out = []
    for shape, axis in SEQUENTIAL + PAIRWISE:
        out += [(shape, axis), (shape, axis - len(shape))]
    out += [((3, c), -1) for c in LAST_COLS]
    out.append((MANY_ROWS, -1))
    return out


def applies(op, shape):
    """LayerNormalization runs on the rank-3 and rank-4 shapes of the table and on every last-axis case."""
    return op != "LayerNormalization" or len(shape) >= 3 or shape[0] == 3 or shape == MANY_ROWS


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _ln_params(rng, shape, axis):
    """gamma and beta of the reduced extent, shaped to broadcast along that axis as NumPy does."""
    axis %= len(shape)
    pshape = (shape[axis],) + (1,) * (len(shape) - 1 - axis)
    gamma = (1 + 0.25 * rng.standard_normal(pshape)).astype(F32)
    beta = (0.5 * rng.standard_normal(pshape)).astype(F32)
    return gamma, beta


def op_inputs(op, x, gamma=None, beta=None, axis=-1):
    """(onnx op, tagged inputs, attrs) of one of REDUCE_OPS."""
    if op.startswith("ReduceMean"):
        return "ReduceMean", [O.F(x)], {"axis": axis, "keepdims": int(op[-1])}
    if op == "Softmax":
        return "Softmax", [O.F(x)], {"axis": axis}
    return "LayerNormalization", [O.F(x), O.F(gamma), O.F(beta)], {"axis": axis, "epsilon": EPS}


def _differ(a, b):
    return np.mean(a.view(np.int32) != b.view(np.int32))


@functools.lru_cache(maxsize=None)
def _reduce_data(shape, axis):
    """x = standard_normal * 3 (contiguous) with gamma and beta.  For a sequential case the first
    draw is taken on which the two orders of summation differ in at least half of the outputs of
    ReduceMean and of Softmax alike — judged on NumPy alone; a test on data without that
    property could not tell the orders apart."""
    for attempt in range(100):
        rng = _rng("reduce", shape, axis, attempt)
        x = (rng.standard_normal(shape) * 3).astype(F32)
        gamma, beta = _ln_params(rng, shape, axis)
        cases = [op_inputs(op, x, axis=axis) for op in ("ReduceMean1", "Softmax")]
        if (shape, axis) not in SEQUENTIAL or all(
                _differ(with_sum(*c, sequential_sum), with_sum(*c, pairwise_sum)) >= 0.5 for c in cases):
            return _frozen(x), _frozen(gamma), _frozen(beta)
    raise AssertionError(f"no data for {shape}, axis {axis} on which the summation orders differ")


@functools.lru_cache(maxsize=None)
def reduce_case(op, shape, axis):
    """(onnx op, inputs, attrs, reference outputs); both spellings of an axis share the data."""
    x, gamma, beta = _reduce_data(shape, axis % len(shape))
    name, ins, attrs = op_inputs(op, x, gamma, beta, axis)
    with np.errstate(all="ignore"):
        ref = O._float_op(name, ins, attrs)
    return name, ins, attrs, [(k, _frozen(a)) for k, a in ref]


def sequential_sum(x, axis):
    """(((+0 + x[0]) + x[1]) + ...) along `axis` in float32, keepdims."""
    acc = np.zeros(x.shape[:axis] + x.shape[axis + 1:], F32)
    for k in range(x.shape[axis]):
        acc = acc + np.take(x, k, axis)
    return np.expand_dims(acc, axis)


def pairwise_sum(x, axis):
    """Move the axis last, copy, sum over the last axis (pairwise in NumPy), keepdims."""
    moved = np.ascontiguousarray(np.moveaxis(x, axis, -1))
    return np.expand_dims(moved.sum(axis=-1), axis)


def with_sum(op, ins, attrs, sum_fn):
    """The reference chain of one of the reduction ops with its sums taken by `sum_fn`."""
    x = ins[0][1]
    axis = attrs["axis"] % x.ndim
    n = F32(x.shape[axis])
    if op == "ReduceMean":
        m = sum_fn(x, axis) / n
        return m if attrs["keepdims"] else np.squeeze(m, axis)
    if op == "Softmax":
        e = np.exp(x + (-x.max(axis=axis, keepdims=True)))
        return e / sum_fn(e, axis)
    mean = sum_fn(x, axis) / n
    dev = x + (-mean)
    var = sum_fn(dev * dev, axis) / n
    std = np.sqrt(var + F32(attrs["epsilon"]))
    return (dev * (F32(1) / std)) * ins[1][1] + ins[2][1]


# ----------------------------------------------------------------------------- (b) special rows
SPECIAL_COLS = (5, 16, 197)
# rows of special_rows(), in the order of the list they restate
ROW_NEG_ZERO, ROW_CONST, ROW_HUGE, ROW_SUBNORMAL, ROW_NAN, ROW_ALL_NINF, ROW_PINF, ROW_MASKED = range(8)


@functools.lru_cache(maxsize=None)
def special_rows(cols):
    rng = _rng("special", cols)
    x = (rng.standard_normal((8, cols)) * 3).astype(F32)
    x[ROW_NEG_ZERO] = -0.0  # NumPy's sum starts from +0: the mean is +0.0
    x[ROW_CONST] = 1.5  # variance exactly 0
    x[ROW_HUGE] = 0.0
    x[ROW_HUGE, cols // 2] = 3e19  # its square overflows
    x[ROW_SUBNORMAL] = np.geomspace(1e-45, 1e-39, cols).astype(F32)
    x[ROW_NAN, cols // 3] = np.nan
    x[ROW_ALL_NINF] = -np.inf
    x[ROW_PINF, cols - 1] = np.inf
    x[ROW_MASKED, ::3] = -np.inf  # masked attention: some -inf, the rest finite
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def special_case(op, cols):
    rng = _rng("special-ln", cols)
    x = special_rows(cols)
    gamma, beta = _ln_params(rng, x.shape, -1)
    gamma[0], beta[0] = 1.25, -0.0  # a -0 product plus -0 keeps its sign: shows the sign of x - mean
    name, ins, attrs = op_inputs(op, x, _frozen(gamma), _frozen(beta), -1)
    with np.errstate(all="ignore"):
        ref = O._float_op(name, ins, attrs)
    return name, ins, attrs, [(k, _frozen(a)) for k, a in ref]


# ----------------------------------------------------------------------------- (c) unary
_POS = [0.0, 1e-45, 1e-40, 1.1754942e-38, 1e-38, 1.0, 88.7, 104.0, 3.4e38, np.inf,
        0.1, 0.5, 2.0, 3.0, 4.0, 5.5, 9.0, 10.0, 20.0, 87.3, 88.72284, 103.97, 1e-30, 1e30, 1e-5]
SPECIALS = _frozen(np.array(_POS + [-v for v in _POS] + [np.nan], F32))
UNARY_LEN = 4099  # odd: the grid-stride tail


@functools.lru_cache(maxsize=None)
def unary_input():
    rng = _rng("unary")
    bits = rng.integers(0, 1 << 32, size=2000, dtype=np.uint64).astype(np.uint32).view(F32)
    x = np.concatenate([SPECIALS, np.linspace(-12, 12, 2048, dtype=F32), bits])
    assert x.size == UNARY_LEN and x.dtype == F32
    return _frozen(x)


def unary_ref(name, x):
    """Bit-exact references: _float_op for the ONNX ops, the reference's expression otherwise."""
    with np.errstate(all="ignore"):
        if name in ("Erf", "Relu", "Sigmoid"):
            return O._float_op(name, [O.F(x)], {})[0][1]
        return {"sqrt": np.sqrt, "inv": lambda v: 1 / v, "exp": np.exp, "neg": lambda v: -v}[name](x)


# NumPy's float32 tanh against tanh in float64: at most 1.36 ulp over linspace(-10, 10, 2^20)
# (measured on the host, tests/test_op_cases_ref.py re-measures it).  The device library's tanhf
# is held to one ulp more: both are faithful-rounding-class implementations, and the claim is
# "as good as what the reference runs".
TANH_NUMPY_ULP = 1.36
TANH_BOUND_ULP = TANH_NUMPY_ULP + 1.0
# tanh(10) = 1 - 4.1e-9, and the float32 below 1 is 6e-8 away: from |x| = 10 on every
# correctly and every faithfully rounded float32 tanh is exactly +-1
TANH_SATURATED = 10.0


def tanh_ulp_error(x, got):
    """(errors in ulp of the float64 reference rounded to float32, mask of the inputs measured)."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        ref = np.tanh(x.astype(np.float64))
        mask = np.isfinite(x)
        ulp = np.spacing(np.abs(ref.astype(F32))).astype(np.float64)
        err = np.abs(np.asarray(got, F32).astype(np.float64) - ref) / ulp
    return err, mask


# ----------------------------------------------------------------------------- (d) binary
BROADCASTS = [((4, 1, 6, 1, 5), (1, 3, 1, 2, 5)),  # five dimensions, none mergeable
              ((2, 3, 4), (2, 3, 4)),  # merges into one
              ((7, 1, 1), (1, 1, 9)),
              ((), (2, 3, 4, 5)), ((2, 3, 4, 5), ())]  # a rank-0 operand


@functools.lru_cache(maxsize=None)
def broadcast_pair(sa, sb):
    rng = _rng("binary", sa, sb)
    a = (rng.standard_normal(sa) * 3).astype(F32)
    b = (rng.standard_normal(sb) * 3).astype(F32)
    b = np.where(np.abs(b) < 0.05, F32(0.05), b).astype(F32)  # a finite quotient
    return _frozen(a), _frozen(b)


def special_pairs():
    """[(a, b)]: every special against every special, and the unary vector against itself
    reversed: 0/0, inf - inf, x/0, 0 * inf, subnormal and overflowing results."""
    v = unary_input()
    return [(_frozen(SPECIALS.reshape(-1, 1)), _frozen(SPECIALS.reshape(1, -1))), (v, _frozen(v[::-1]))]


def binary_ref(name, a, b):
    with np.errstate(all="ignore"):
        if name == "Sub":  # the reference has no Sub: a + (-b)
            return a + (-b)
        return O._float_op(name, [O.F(a), O.F(b)], {})[0][1]


SCALARS = (1e-12, 0.5, -3.0e38)


# ----------------------------------------------------------------------------- (e) structural
@functools.lru_cache(maxsize=None)
def struct_array(shape, key="struct"):
    return _frozen((_rng(key, shape).standard_normal(shape) * 3).astype(F32))


I64_MAX = np.iinfo(np.int64).max
GATHER = [  # (index array, axis) on a (5, 6, 7) input
    (np.array(2), 0), (np.array(-1), 1), (np.array([4, 0, 0, -5]), 0), (np.array([1, -6, 5]), 1),
    (np.array([[0, 6], [-7, 3], [2, 2]]), -1), (np.array([[1, -1]]), 1)]
GATHER_BAD = [(np.array([0, 5]), 0), (np.array(-7), 1), (np.array([[7]]), -1)]
SLICE = [  # (starts, ends, axes) on a (5, 6, 7) input
    ([1], [I64_MAX], [1]), ([-3], [I64_MAX], [2]), ([-4], [-1], [0]), ([3], [3], [1]), ([4], [2], [2]),
    ([1, -5], [4, I64_MAX], [0, 2]), ([0, 2], [I64_MAX, 5], [2, 1])]


def slice_index(spec, ndim):
    """The index tuple the Slice op builds from (starts, ends, axes) (model.py:182-190)."""
    sl = [slice(None)] * ndim
    for s, e, a in zip(*spec):
        sl[a] = slice(s, e)
    return tuple(sl)


CONCAT = [(((2, 3, 4), (5, 3, 4), (1, 3, 4)), 0), (((2, 3, 4), (2, 1, 4), (2, 6, 4)), 1),
          (((2, 3, 4), (2, 3, 1), (2, 3, 7)), -1)]
EXPAND = [((3, 1, 5), [1, 4, 1]),  # target 1 keeps the extent
          ((3, 1, 5), [3, 4, 5]), ((1, 1), [6, 7]), ((2, 3), [1, 1])]
WHERE = [((4, 1, 5), (1, 3, 5), (4, 3, 1), "mixed"), ((1, 6), (5, 1), (5, 6), "mixed"),
         ((2, 3), (2, 3), (2, 3), "true"), ((3,), (2, 3), (1,), "false")]  # cond, a, b shapes
QBITS = (8, 12, 32, 40)  # storage of 1, 2, 4 and 8 bytes


@functools.lru_cache(maxsize=None)
def qtensor_data(bit_width, shape=(3, 5, 7)):
    """int64 values over the whole range of the bit width, both ends included."""
    lo, hi = -(1 << (bit_width - 1)), (1 << (bit_width - 1)) - 1
    q = _rng("q", bit_width, shape).integers(lo, hi, size=shape, endpoint=True, dtype=np.int64)
    q.flat[0], q.flat[-1] = lo, hi
    return _frozen(q)
