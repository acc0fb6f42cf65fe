"""GPU parity of the per-node integer path, kernel by kernel: nqk_quantize, nqk_dequantize,
nqk_requantize, nqk_rowsum, nqk_relu_q, nqk_qgemm_i8 and nqk_qgemm_generic through
numpy_quant.kernels, QTensor and numpy_quant.numpy_quantization, against the oracle's NumPy
restatement on the same host arrays.  This is the path every fused kernel is checked against.
Every comparison is exact: assert_array_equal on integers, on the int32 view of floats; storage
dtypes and kernel routes are asserted too.  The inputs, their references and the edges they reach
are tests/_l1_cases.py (asserted without a GPU by tests/test_l1_cases_ref.py).

Not covered, by decision: NaN quantized into narrow storage (it keeps INT64_MIN's low bits, 0),
bit widths 33-64, more than 65535 matrices in one product (an error)."""
import numpy as np
import pytest

import _l1_cases as C
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
I64 = np.int64


class _Dev:
    def __init__(self):
        from numpy_quant import _lib, device, kernels, numpy_quantization, tensor
        _lib.ensure_init()
        self.lib, self.K, self.nq, self.T = _lib, kernels, numpy_quantization, tensor
        self.Array = device.DeviceArray


@pytest.fixture(scope="module")
def dev():
    return _Dev()


def same_bits(got, ref, what=""):
    assert got.dtype == F32 and ref.dtype == F32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(ref).view(np.int32),
                                  err_msg=str(what))


def same_ints(got, ref, what=""):
    assert got.dtype == I64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    np.testing.assert_array_equal(got, ref, err_msg=str(what))


def expected_storage(bw, ref, no_zp):
    """storage_dtype(bw); int64 only where the reference holds the float32 bound 2^31 (bit width 32
    without a zero point)."""
    st = C.storage(bw)
    if bw == 32 and no_zp and ref.size and ref.max() > np.iinfo(np.int32).max:
        return np.dtype(np.int64)
    return st


# ----------------------------------------------------------------------------- group 1: quantize
@pytest.mark.parametrize("qp", C.QPARAMS, ids=lambda p: f"s{p[0]}-zp{p[1]}")
@pytest.mark.parametrize("bw", C.BIT_WIDTHS)
def test_quantize_int64(dev, bw, qp):
    """nq.quantize (int64 storage), NaN included: NaN -> INT64_MIN."""
    scale, zp = qp
    out = dev.nq.quantize(C.quant_input(bw, scale, zp), bw, np.array(scale, F32), C.zp_arr(zp))
    same_ints(out, C.quant_ref(bw, scale, zp), (bw, scale, zp))


@pytest.mark.parametrize("qp", C.QPARAMS, ids=lambda p: f"s{p[0]}-zp{p[1]}")
@pytest.mark.parametrize("bw", C.BIT_WIDTHS)
def test_quantize_narrow(dev, bw, qp):
    """K.quantize and quantize_tensor in their default storage, NaN left out.  At bit width 32
    without a zero point the reference saturates at float32(2^31 - 1) = +2^31."""
    scale, zp = qp
    x = C.quant_input(bw, scale, zp)
    keep = ~np.isnan(x)
    x, ref = np.ascontiguousarray(x[keep]), C.quant_ref(bw, scale, zp)[keep]
    q, rs = dev.K.quantize(dev.Array.from_host(x), bw, scale, zp)
    assert rs is None and q.dtype == expected_storage(bw, ref, zp is None), (bw, scale, zp, q.dtype)
    same_ints(q.to_host().astype(I64), ref, (bw, scale, zp))
    t = dev.T.quantize_tensor(dev.T.FTensor(x), bw, np.array(scale, F32), C.zp_arr(zp))
    assert t.dev.dtype == q.dtype and t.bit_width == bw
    same_ints(t.data, ref, (bw, scale, zp, "quantize_tensor"))


def test_quantize_32_bits_stays_int32_when_nothing_saturates(dev):
    x = np.array([-3e9, -2147483648.0, -5.5, 0.0, 2.5, 2147483520.0], F32)  # the largest float32 below 2^31
    q, _ = dev.K.quantize(dev.Array.from_host(x), 32, 1.0, None)
    assert q.dtype == np.int32
    same_ints(q.to_host().astype(I64), C.quantize_ref(x, 32, 1.0, None))


@pytest.mark.parametrize("n", C.FLAT_N)
def test_quantize_flat_lengths(dev, n):
    bw, scale, zp = C.FLAT_QP
    x = C.flat_input(n)
    q, _ = dev.K.quantize(dev.Array.from_host(x), bw, scale, zp)
    assert q.dtype == np.int8 and q.shape == (n,)
    same_ints(q.to_host().astype(I64), C.quantize_ref(x, bw, scale, zp), n)


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_quantize_flat_unaligned(dev, offset):
    """A view 4, 8 or 12 bytes into its buffer: the scalar branch for heads that are not 16-byte aligned."""
    bw, scale, zp = C.FLAT_QP
    host = C.flat_input(C.UNALIGNED_N + 3)
    base = dev.Array.from_host(host)
    assert base.ptr % 16 == 0
    view = base.offset_view(offset, (C.UNALIGNED_N,))
    q, _ = dev.K.quantize(view, bw, scale, zp)
    same_ints(q.to_host().astype(I64), C.quantize_ref(host[offset:offset + C.UNALIGNED_N], bw, scale, zp), offset)


@pytest.mark.parametrize("qp", C.ROW_QP, ids=lambda p: f"bw{p[0]}-zp{p[2]}")
@pytest.mark.parametrize("shape", C.ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantize_rows_with_rowsum(dev, shape, qp):
    bw, scale, zp = qp
    x = C.row_input(*shape)
    ref = C.quantize_ref(x, bw, scale, zp)
    q, rs = dev.K.quantize(dev.Array.from_host(x), bw, scale, zp, rowsum=True)
    assert q.dtype == C.storage(bw) and q.shape == shape and rs.shape == shape[:1] and rs.dtype == I64
    same_ints(q.to_host().astype(I64), ref, (shape, qp))
    same_ints(rs.to_host(), ref.sum(-1), (shape, qp, "rowsum"))


# ----------------------------------------------------------------------------- group 2: de/requantize
@pytest.mark.parametrize("form", C.ZP_FORMS)
def test_big_accumulators(dev, form):
    """Accumulators around 2^24, 2^31, 2^53 and 2^62: the int64 subtraction of the zero point is
    exact, the int64 -> float64 conversion rounds to even."""
    acc, zp = C.big_acc(), C.zp_form(form, C.BIG_SHAPE)
    same_bits(dev.nq.dequantize(acc, C.BIG_SCALE, zp), O.dequantize(acc, C.BIG_SCALE, zp), form)
    for bw in (8, 32):
        for rz in (None, -3):
            ref = O.requantize(acc, C.BIG_SCALE, zp, C.BIG_RES_SCALE, C.zp_arr(rz), bw)
            same_ints(dev.nq.requantize(acc, C.BIG_SCALE, zp, C.BIG_RES_SCALE, C.zp_arr(rz), bw), ref, (form, bw, rz))


@pytest.mark.parametrize("rz", C.TIE_RES_ZP)
@pytest.mark.parametrize("bw", C.TIE_BW)
def test_requantize_ties_and_clips(dev, bw, rz):
    """acc * 0.5 / 1 is exactly k + 0.5 on the odd accumulators: rint is half-even; both clips."""
    acc = C.tie_acc(bw)
    ref = O.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, C.zp_arr(rz), bw)
    same_ints(dev.nq.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, C.zp_arr(rz), bw), ref, (bw, rz))
    q = dev.K.requantize(dev.Array.from_host(acc), C.TIE_ARR_SCALE, None, None, C.TIE_RES_SCALE, rz, bw)
    assert q.dtype == expected_storage(bw, ref, rz is None), (bw, rz, q.dtype)
    same_ints(q.to_host().astype(I64), ref, (bw, rz, "narrow"))


def test_requantize_32_bits_without_zero_point(dev):
    """The reference's result reaches +2^31 (float32 clip); int32 storage would flip its sign."""
    acc = C.sat32_acc()
    ref = O.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, None, 32)
    q = dev.K.requantize(dev.Array.from_host(acc), C.TIE_ARR_SCALE, None, None, C.TIE_RES_SCALE, None, 32)
    same_ints(q.to_host().astype(I64), ref)
    t = dev.T.QTensor(np.array(acc), 64, C.TIE_ARR_SCALE, None).requantize(32, C.TIE_RES_SCALE, None)
    same_ints(t.data, ref, "QTensor")
    # with a zero point the clip is in float64 and 2^31 - 1 exact; nothing saturating stays int32
    ref = O.requantize(acc, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, C.zp_arr(-3), 32)
    q = dev.K.requantize(dev.Array.from_host(acc), C.TIE_ARR_SCALE, None, None, C.TIE_RES_SCALE, -3, 32)
    assert q.dtype == np.int32
    same_ints(q.to_host().astype(I64), ref)
    small = np.array([5, -7, 2 ** 31 - 300, -2 ** 32], I64)
    q = dev.K.requantize(dev.Array.from_host(small), C.TIE_ARR_SCALE, None, None, C.TIE_RES_SCALE, None, 32)
    assert q.dtype == np.int32
    same_ints(q.to_host().astype(I64), O.requantize(small, C.TIE_ARR_SCALE, None, C.TIE_RES_SCALE, None, 32))


def test_elementwise_grid_stride(dev):
    """1049 x 1001 elements, more than 4096 blocks of 256 threads: the loops go round."""
    acc, zp = C.stride_acc()
    s, rs = F32(0.0047), F32(30)
    same_bits(dev.nq.dequantize(acc, s, zp), O.dequantize(acc, s, zp))
    same_ints(dev.nq.requantize(acc, s, zp, rs, C.zp_arr(-3), 8), O.requantize(acc, s, zp, rs, C.zp_arr(-3), 8))


# ----------------------------------------------------------------------------- group 3: matmul
@pytest.mark.parametrize("bw", C.MM_BW)
@pytest.mark.parametrize("name", C.MM_NAMES)
def test_matmul_dequantize_requantize(dev, name, bw):
    """QTensor.matmul -> dequantize / (+ bias).requantize with the zero-point term kept on the
    device as row and column sums (ZP_ROW / ZP_COL / ZP_KCONST through the batch map)."""
    QTensor = dev.T.QTensor
    _, sa, sb, weight = C.mm_shape(name)
    mfma = bw <= 8 and "generic" not in name
    for zpair in C.ZP_PAIRS:
        case = C.mm_case(name, bw, zpair)
        what = (name, bw, zpair)
        A = QTensor(np.array(case["a"]), bw, C.MM_SA, C.zp_arr(case["za"]))
        B = QTensor(np.array(case["b"]), bw, C.MM_SB, C.zp_arr(case["zb"]))
        assert A.dev.dtype == B.dev.dtype == C.storage(bw)
        B._is_weight = weight
        for _ in range(2 if weight else 1):  # the second product reads the cached operand and column sums
            acc = A.matmul(B)
            assert (B._bt is not None) == (weight and bw <= 8)
            assert acc.dev.dtype == (np.int32 if mfma else np.int64), (what, acc.dev.dtype)
            assert acc.bit_width == 4 * bw and acc.scale == case["s"] and acc.shape == case["acc"].shape
            same_ints(acc.data, case["acc"], what)
            if case["term"] is None:
                assert acc.zero_point is None
            else:
                same_ints(np.ascontiguousarray(np.broadcast_to(acc.zero_point, acc.shape)),
                          np.broadcast_to(case["term"], acc.shape), (what, "term"))
            same_bits(acc.dequantize().data, case["deq"], what)
            for kind in C.BIASES:
                bias = case["biases"][kind]
                if kind == "none":
                    biased = acc
                elif kind == "vector":
                    bq = QTensor(np.array(bias), 4 * bw, case["s"], None)
                    assert bq.dev.dtype == C.storage(4 * bw)
                    biased = acc + bq
                else:
                    biased = acc + QTensor(dev.Array.from_host(bias.astype(np.int8)), 4 * bw, case["s"], None)
                for rz in C.MM_RES_ZP:
                    rs, ref = case["requant"][kind, rz]
                    out = biased.requantize(bw, rs, C.zp_arr(rz))
                    assert out.dev.dtype == C.storage(bw) and out.bit_width == bw
                    same_ints(out.data, ref, (what, kind, rz))


@pytest.mark.parametrize("i", range(len(C.MIXED)), ids=lambda i: "x".join(np.dtype(t).name for t in C.MIXED[i][::2]))
def test_generic_gemm_mixed_storage(dev, i):
    """nqk_qgemm_generic with operands of two storages; sums beyond 2^53 stay exact in int64."""
    a, b, ref = C.mixed_case(i)
    (m, k), n = a.shape, b.shape[1]
    da, db = dev.Array.from_host(a), dev.Array.from_host(b)
    out = dev.Array((m, n), I64)
    dev.lib.call("nqk_qgemm_generic", da.vp, da.code, db.vp, db.code, out.vp, 1, m, n, k, k, 1, n, 1, n,
                 dev.lib.i64arr(dev.K.batch_map((), ())[1]), m * k, k * n, m * n)
    same_ints(out.to_host(), ref)


# ----------------------------------------------------------------------------- group 4: accumulator width
@pytest.mark.parametrize("zpair", C.ACC_ZP, ids=("nozp", "zp"))
@pytest.mark.parametrize("k", C.ACC_K)
def test_long_k_products_are_exact(dev, k, zpair):
    """int8 x int8 with K up to and past 2^17, where 2^14 * K no longer fits an int32 accumulator."""
    a, b, ref, s, term = C.acc_case(k, zpair)
    za, zb = (C.zp_arr(z) for z in zpair)
    acc, scale, zt = dev.nq.q_matmul(a, C.MM_SA, za, b, C.MM_SB, zb)
    same_ints(acc, ref, (k, "q_matmul"))
    assert F32(scale) == s
    A = dev.T.QTensor(np.array(a), 8, C.MM_SA, za)
    B = dev.T.QTensor(np.array(b), 8, C.MM_SB, zb)
    assert A.dev.dtype == B.dev.dtype == np.int8
    out = A.matmul(B)
    same_ints(out.data, ref, (k, "QTensor"))
    B._is_weight = True  # and with the cached transposed operand and column sums
    outw = A.matmul(B)
    same_ints(outw.data, ref, (k, "QTensor, weight"))
    if term is None:
        assert zt is None and out.zero_point is None and outw.zero_point is None
    else:
        for z in (zt, out.zero_point, outw.zero_point):
            same_ints(np.ascontiguousarray(np.broadcast_to(z, ref.shape)), np.broadcast_to(term, ref.shape), k)
        same_bits(outw.dequantize().data, O.dequantize(ref, s, term), k)


def test_int8_gemm_refuses_a_k_it_cannot_hold(dev):
    k = (1 << 17) + 16
    a, bt, c = dev.Array((1, k), np.int8).fill_zero(), dev.Array((1, k), np.int8).fill_zero(), dev.Array((1, 1), np.int32)
    with pytest.raises(dev.lib.NQKError, match="int32 accumulator"):
        dev.lib.call("nqk_qgemm_i8", a.vp, bt.vp, c.vp, 1, 1, 1, k, k, k, 1, None, k, k, 1)


# ----------------------------------------------------------------------------- group 5: relu_q, rowsum
@pytest.mark.parametrize("n", C.RELU_N)
@pytest.mark.parametrize("dt", C.RELU_DTYPES, ids=lambda t: np.dtype(t).name)
def test_relu_q(dev, dt, n):
    bits = 8 * np.dtype(dt).itemsize
    for zp, outside in C.relu_zero_points(dt):
        q, ref = C.relu_case(dt, n, zp)
        out = dev.T.QTensor(dev.Array.from_host(q), bits, F32(0.1), C.zp_arr(zp)).relu()
        assert out.dev.dtype == (np.int64 if outside else dt), (dt, n, zp, out.dev.dtype)
        assert out.zero_point == zp and out.bit_width == bits
        same_ints(out.data, ref, (dt, n, zp))


@pytest.mark.parametrize("shape", C.ROWSUM_SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("dt", C.RELU_DTYPES, ids=lambda t: np.dtype(t).name)
def test_rowsum(dev, dt, shape):
    """Row sums of padded rows (ld > k) in padded matrices (bstride > rows * ld)."""
    buf, ref = C.rowsum_case(dt, shape)
    out = dev.K.rowsum(dev.Array.from_host(buf), *shape)
    assert out.shape == ref.shape
    same_ints(out.to_host(), ref, (dt, shape))
