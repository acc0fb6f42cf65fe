"""Typed wrappers around the libnqk.so entry points, on DeviceArrays.

One function per kernel family; argument checking (shapes the kernels and their
grids assume) happens here, on the host, before anything is launched.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from . import _lib
from .device import (DeviceArray, broadcast_strides, collapse, contiguous_strides, copy_strided,
                     materialize_broadcast)

VP = ctypes.c_void_p


def storage_dtype(bit_width: int) -> np.dtype:
    """Narrowest integer storage for values in [-2^(bw-1), 2^(bw-1)-1]."""
    if bit_width <= 8:
        return np.dtype(np.int8)
    if bit_width <= 16:
        return np.dtype(np.int16)
    if bit_width <= 32:
        return np.dtype(np.int32)
    return np.dtype(np.int64)


def _f32_bound_exceeds(bit_width: int, zp) -> bool:
    """Without a zero point the reference clips in float32, and float32(2^31 - 1) is 2^31: at
    bit width 32 the upper bound itself does not fit the int32 storage of that width.  (For
    25..31 bits the rounded bound 2^(bw-1) still fits; with a zero point the clip is in
    float64 and exact.)"""
    return zp is None and bit_width == 32


def _narrow_if_fits(q: DeviceArray, dt: np.dtype) -> DeviceArray:
    """An int64 result in storage `dt` when every value fits it, else as it is.  One download
    and one upload: this runs for biases when a model is built, not per forward."""
    h = q.to_host()
    info = np.iinfo(dt)
    if h.size and (h.min() < info.min or h.max() > info.max):
        return q
    return DeviceArray.from_host(h.astype(dt))


# ----------------------------------------------------------------------------- quantization
def quantize(x: DeviceArray, bit_width: int, scale: float, zp: int | None, out_dtype=None,
             rowsum: bool = False):
    """numpy_quantization.py:24-34 on device.  Returns (q, rowsum | None).  Storage is
    `out_dtype`, else `storage_dtype(bit_width)`; the one exception is bit width 32 without a
    zero point, whose saturated value +2^31 needs int64 (int32 whenever nothing saturates)."""
    if x.dtype != np.float32:
        raise ValueError("quantize expects float32 input")
    dt = np.dtype(out_dtype) if out_dtype is not None else storage_dtype(bit_width)
    widen = out_dtype is None and _f32_bound_exceeds(bit_width, zp)
    q = DeviceArray(x.shape, np.int64 if widen else dt)
    rs = None
    row_len = x.shape[-1] if x.ndim else 1
    if rowsum:
        rs = DeviceArray(x.shape[:-1] if x.ndim else (), np.int64)
    _lib.call("nqk_quantize", x.vp, q.vp, q.code, x.size, float(np.float32(scale)),
              0 if zp is None else int(zp), 0 if zp is None else 1, int(bit_width),
              rs.vp if rs is not None else None, row_len)
    if widen:
        q = _narrow_if_fits(q, dt)
    return q, rs


class ZpTerm:
    """Zero-point term of a q_matmul output (numpy_quantization.py:49-61), kept as
    row sums of A and column sums of B instead of an int64 (..., M, N) array."""

    __slots__ = ("flags", "zpa", "zpb", "K", "row", "col", "bmap", "a_batch", "b_batch", "M", "N")

    def __init__(self, flags, zpa, zpb, K, row, col, bmap, a_batch, b_batch, M, N):
        self.flags, self.zpa, self.zpb, self.K = flags, zpa, zpb, K
        self.row, self.col, self.bmap = row, col, bmap
        self.a_batch, self.b_batch, self.M, self.N = tuple(a_batch), tuple(b_batch), M, N

    def to_host(self) -> np.ndarray:
        """The reference's int64 zero_point array (same shape and values)."""
        term = None
        if self.flags & _lib.ZP_ROW:
            term = self.row.to_host().reshape(self.a_batch + (self.M, 1)) * np.int64(self.zpb)
        if self.flags & _lib.ZP_COL:
            c = self.col.to_host().reshape(self.b_batch + (1, self.N)) * np.int64(self.zpa)
            term = c if term is None else term + c
        if self.flags & _lib.ZP_KCONST:
            term = term - np.int64(self.zpa) * np.int64(self.zpb) * np.int64(self.K)
        return term


def _zp_args(zp):
    """(flags, zp, zpa, zpb, K, row, col, bmap) for dequantize / requantize."""
    if zp is None:
        return _lib.ZP_NONE, 0, 0, 0, 0, None, None, None
    if isinstance(zp, ZpTerm):
        return (zp.flags, 0, zp.zpa, zp.zpb, zp.K, zp.row.vp if zp.row is not None else None,
                zp.col.vp if zp.col is not None else None, _lib.i64arr(zp.bmap))
    return _lib.ZP_SCALAR, int(zp), 0, 0, 0, None, None, None


def _bmn(shape):
    if isinstance(shape, tuple) and len(shape) >= 2:
        return int(math.prod(shape[:-2])), int(shape[-2]), int(shape[-1])
    return 1, 1, int(math.prod(shape))


def dequantize(q: DeviceArray, scale, zp) -> DeviceArray:
    """f32( f64(q - zp) * f64(s) )  (numpy_quantization.py:37-41, tensor.py:261-265)."""
    out = DeviceArray(q.shape, np.float32)
    flags, z, zpa, zpb, K, row, col, bmap = _zp_args(zp)
    if isinstance(zp, ZpTerm):
        b, m, n = _bmn(q.shape)
    else:
        b, m, n = 1, 1, q.size
    _lib.call("nqk_dequantize", q.vp, q.code, out.vp, b, m, n, float(np.float32(scale)), flags, z, zpa, zpb,
              K, row, col, bmap)
    return out


def requantize(acc: DeviceArray, scale, zp, bias: DeviceArray | None, res_scale, res_zp,
               bit_width: int) -> DeviceArray:
    """numpy_quantization.py:64-72 with the Gemm bias add (tensor.py:255-259) fused.  Storage as
    for `quantize`: int64 at bit width 32 without a result zero point where +2^31 occurs."""
    dt = storage_dtype(bit_width)
    widen = _f32_bound_exceeds(bit_width, res_zp)
    out = DeviceArray(acc.shape, np.int64 if widen else dt)
    flags, z, zpa, zpb, K, row, col, bmap = _zp_args(zp)
    b, m, n = _bmn(acc.shape) if acc.ndim >= 2 else (1, 1, acc.size)
    if bias is not None and bias.size != n:
        raise ValueError(f"bias of {bias.size} elements cannot broadcast over rows of {n}")
    _lib.call("nqk_requantize", acc.vp, acc.code, bias.vp if bias is not None else None,
              bias.code if bias is not None else _lib.NQK_I64, out.vp, out.code, b, m, n,
              float(np.float32(scale)), flags, z, zpa, zpb, K, row, col, bmap,
              float(np.float32(res_scale)), 0 if res_zp is None else int(res_zp),
              0 if res_zp is None else 1, int(bit_width))
    return _narrow_if_fits(out, dt) if widen else out


# ----------------------------------------------------------------------------- per-column scales
def is_cols(scale) -> bool:
    """Whether a scale is a per-column vector (QModel.per_channel) rather than a scalar."""
    return np.ndim(scale) == 1


def _check_cols(scale: DeviceArray, n: int, what: str) -> None:
    if not isinstance(scale, DeviceArray) or scale.dtype != np.float32 or scale.shape != (n,):
        raise ValueError(f"{what}: the scale vector must be a float32 DeviceArray [{n}]")


def minmax_cols(x: DeviceArray) -> tuple[np.ndarray, np.ndarray]:
    """(min, max) float32 [cols] of every column of a 2-D float32 array (nqk_minmax_cols)."""
    if x.dtype != np.float32 or x.ndim != 2 or x.size == 0:
        raise ValueError("minmax_cols expects a non-empty 2-D float32 array")
    rows, cols = x.shape
    res = DeviceArray((2, cols), np.float32)
    _lib.call("nqk_minmax_cols", x.vp, rows, cols, cols, res.vp)
    h = res.to_host()
    return h[0], h[1]


def quantize_cols(x: DeviceArray, bit_width: int, scale: DeviceArray, out_dtype=None) -> DeviceArray:
    """numpy_quantization.py:24-34 without a zero point, the scale of column n = scale[n]
    (nqk_quantize_cols).  Storage as `quantize` chooses it."""
    if x.dtype != np.float32 or x.ndim < 1:
        raise ValueError("quantize_cols expects a float32 array of at least one dimension")
    cols = x.shape[-1]
    _check_cols(scale, cols, "quantize_cols")
    dt = np.dtype(out_dtype) if out_dtype is not None else storage_dtype(bit_width)
    widen = out_dtype is None and _f32_bound_exceeds(bit_width, None)
    q = DeviceArray(x.shape, np.int64 if widen else dt)
    _lib.call("nqk_quantize_cols", x.vp, q.vp, q.code, x.size // cols if cols else 0, cols, scale.vp, int(bit_width))
    return _narrow_if_fits(q, dt) if widen else q


def dequantize_cols(q: DeviceArray, scale: DeviceArray, zp) -> DeviceArray:
    """`dequantize` with scale[n] over the last axis (nqk_dequantize_cols)."""
    if q.ndim < 1:
        raise ValueError("dequantize_cols expects at least one dimension")
    _check_cols(scale, q.shape[-1], "dequantize_cols")
    out = DeviceArray(q.shape, np.float32)
    flags, z, zpa, zpb, K, row, col, bmap = _zp_args(zp)
    b, m, n = _bmn(q.shape) if q.ndim >= 2 else (1, 1, q.size)
    _lib.call("nqk_dequantize_cols", q.vp, q.code, out.vp, b, m, n, scale.vp, flags, z, zpa, zpb, K, row, col, bmap)
    return out


def requantize_cols(acc: DeviceArray, scale: DeviceArray, zp, bias: DeviceArray | None, res_scale, res_zp,
                    bit_width: int) -> DeviceArray:
    """`requantize` with scale[n] over the last axis (nqk_requantize_cols)."""
    if acc.ndim < 1:
        raise ValueError("requantize_cols expects at least one dimension")
    dt = storage_dtype(bit_width)
    widen = _f32_bound_exceeds(bit_width, res_zp)
    out = DeviceArray(acc.shape, np.int64 if widen else dt)
    flags, z, zpa, zpb, K, row, col, bmap = _zp_args(zp)
    b, m, n = _bmn(acc.shape) if acc.ndim >= 2 else (1, 1, acc.size)
    _check_cols(scale, n, "requantize_cols")
    if bias is not None and bias.size != n:
        raise ValueError(f"bias of {bias.size} elements cannot broadcast over rows of {n}")
    _lib.call("nqk_requantize_cols", acc.vp, acc.code, bias.vp if bias is not None else None,
              bias.code if bias is not None else _lib.NQK_I64, out.vp, out.code, b, m, n, scale.vp,
              flags, z, zpa, zpb, K, row, col, bmap, float(np.float32(res_scale)),
              0 if res_zp is None else int(res_zp), 0 if res_zp is None else 1, int(bit_width))
    return _narrow_if_fits(out, dt) if widen else out


def rowsum(a: DeviceArray, batch: int, rows: int, k: int, ld: int, bstride: int) -> DeviceArray:
    out = DeviceArray((batch * rows,), np.int64)
    _lib.call("nqk_rowsum", a.vp, a.code, out.vp, batch, rows, k, ld, bstride)
    return out


# ----------------------------------------------------------------------------- batch maps
def batch_map(a_batch, b_batch):
    """Express np.matmul batch broadcasting as (out_batch, [inner, ao, ai, bo, bi])
    or None when it cannot be split into two uniform groups."""
    nd = max(len(a_batch), len(b_batch))
    a = (1,) * (nd - len(a_batch)) + tuple(a_batch)
    b = (1,) * (nd - len(b_batch)) + tuple(b_batch)
    out = []
    for x, y in zip(a, b):
        if x != y and x != 1 and y != 1:
            raise ValueError(f"matmul batch shapes {a_batch} and {b_batch} do not broadcast")
        out.append(max(x, y))
    out = tuple(out)

    def group_kind(src, lo, hi):
        full = all(src[k] == out[k] for k in range(lo, hi))
        one = all(src[k] == 1 for k in range(lo, hi))
        return "full" if full else ("one" if one else None)

    for p in range(nd + 1):
        ka_o, ka_i = group_kind(a, 0, p), group_kind(a, p, nd)
        kb_o, kb_i = group_kind(b, 0, p), group_kind(b, p, nd)
        if None in (ka_o, ka_i, kb_o, kb_i):
            continue
        inner = int(math.prod(out[p:]))
        a_inner = int(math.prod(a[p:]))
        b_inner = int(math.prod(b[p:]))
        ao = a_inner if ka_o == "full" else 0
        ai = 1 if ka_i == "full" and a_inner > 1 else 0
        bo = b_inner if kb_o == "full" else 0
        bi = 1 if kb_i == "full" and b_inner > 1 else 0
        return out, [max(inner, 1), ao, ai, bo, bi]
    return out, None


# ----------------------------------------------------------------------------- integer GEMM
MFMA_MIN_WORK = 1 << 15
# nqk_qgemm_i8 accumulates in int32: |a * b| <= 2^14, so K products stay below 2^31 only while
# K < 2^17 (K = 131072 of -128 * -128 is exactly 2^31).  Longer K goes to the int64 kernel.
I8_MAX_K = 1 << 17


class KernelTimer:
    """Brackets selected kernel launches with stream events (bench.py roofline):
    `records` collects (tag, start_event, stop_event, work) tuples."""

    def __init__(self):
        self.records = []
        self._free = []

    def _event(self):
        if self._free:
            return self._free.pop()
        e = ctypes.c_void_p()
        _lib.call("nqk_event_create", ctypes.byref(e))
        return e

    def begin(self):
        e = self._event()
        _lib.call("nqk_event_record", e)
        return e

    def end(self, tag, start, work, unit="int8"):
        """work = (ops, algorithmic bytes); unit: what the ops count ("int8" MFMA ops,
        "flop32" f32 MFMA flops)."""
        e = self._event()
        _lib.call("nqk_event_record", e)
        self.records.append((tag, start, e, work, unit))

    def collect(self):
        """[(tag, ms, work, unit)] and recycle the events."""
        out = []
        for tag, a, b, w, unit in self.records:
            ms = ctypes.c_float()
            _lib.call("nqk_event_elapsed", a, b, ctypes.byref(ms))
            out.append((tag, ms.value, w, unit))
            self._free += [a, b]
        self.records = []
        return out


TIMER: KernelTimer | None = None


def _pad_k(x: DeviceArray, rows_shape, k: int, kp: int) -> DeviceArray:
    """Copy [..., rows, k] into a zero-filled [..., rows, kp] (kp % 16 == 0)."""
    out = DeviceArray(tuple(rows_shape) + (kp,), x.dtype).fill_zero()
    shape = tuple(rows_shape) + (k,)
    copy_strided(x, out, shape, contiguous_strides(shape), contiguous_strides(tuple(rows_shape) + (kp,)))
    return out


def qmatmul(a: DeviceArray, b: DeviceArray, zpa, zpb, b_transposed: DeviceArray | None = None,
            b_colsum: DeviceArray | None = None):
    """q_matmul (numpy_quantization.py:44-61): returns (acc, ZpTerm | None).

    a: [..., M, K] and b: [..., K, N] integer DeviceArrays (contiguous).  The int8
    path needs Bt[..., N, Kp]; `b_transposed` (and its column sums) may be passed in
    pre-computed for constant weights.
    """
    if a.ndim < 2 or b.ndim < 2:
        raise ValueError("q_matmul operands must have at least 2 dimensions")
    M, K = a.shape[-2:]
    K2, N = b.shape[-2:]
    if K != K2:
        raise ValueError(f"matmul: mismatch in core dimension ({K} vs {K2})")
    a_batch, b_batch = a.shape[:-2], b.shape[:-2]
    out_batch, bmap = batch_map(a_batch, b_batch)
    if bmap is None:  # exotic broadcast: materialise both operands
        a = materialize_broadcast(a, out_batch + (M, K))
        b = materialize_broadcast(b, out_batch + (K, N))
        a_batch = b_batch = out_batch
        b_transposed = b_colsum = None
        _, bmap = batch_map(a_batch, b_batch)
    nb = int(math.prod(out_batch))
    na, nbb = int(math.prod(a_batch)), int(math.prod(b_batch))
    use_mfma = (a.dtype == np.int8 and b.dtype == np.int8 and M * N * K >= MFMA_MIN_WORK and nb <= 65535
                and K < I8_MAX_K)
    if use_mfma:
        kp = (K + 15) // 16 * 16
        ap = a if K == kp else _pad_k(a, a.shape[:-1], K, kp)
        if b_transposed is None:
            bt = DeviceArray(b_batch + (N, kp), np.int8)
            if K != kp:
                bt.fill_zero()
            shape = b_batch + (N, K)
            bst = contiguous_strides(b.shape)
            src_st = list(bst[:-2]) + [bst[-1], bst[-2]]
            copy_strided(b, bt, shape, src_st, contiguous_strides(b_batch + (N, kp)))
        else:
            bt = b_transposed
        acc = DeviceArray(out_batch + (M, N), np.int32)
        t0 = TIMER.begin() if TIMER is not None else None
        _lib.call("nqk_qgemm_i8", ap.vp, bt.vp, acc.vp, nb, M, N, kp, kp, kp, N, _lib.i64arr(bmap),
                  M * kp, N * kp, M * N)
        if t0 is not None:
            TIMER.end("qgemm_i8", t0, (2 * nb * M * N * K, nb * (M * K + N * K + 4 * M * N)))
    else:
        acc = DeviceArray(out_batch + (M, N), np.int64)
        _lib.call("nqk_qgemm_generic", a.vp, a.code, b.vp, b.code, acc.vp, nb, M, N, K, K, 1, N, 1, N,
                  _lib.i64arr(bmap), M * K, K * N, M * N)
        bt = None
    if zpa is None and zpb is None:
        return acc, None
    row = col = None
    flags = 0
    if zpb is not None:
        row = rowsum(a, na, M, K, K, M * K)
        flags |= _lib.ZP_ROW
    if zpa is not None:
        if b_colsum is not None:
            col = b_colsum
        elif bt is not None and use_mfma:
            kp = bt.shape[-1]
            col = rowsum(bt, nbb, N, kp, kp, N * kp)
        else:
            btt = DeviceArray(b_batch + (N, K), b.dtype)
            bst = contiguous_strides(b.shape)
            copy_strided(b, btt, b_batch + (N, K), list(bst[:-2]) + [bst[-1], bst[-2]],
                         contiguous_strides(b_batch + (N, K)))
            col = rowsum(btt, nbb, N, K, K, N * K)
        flags |= _lib.ZP_COL
    if zpa is not None and zpb is not None:
        flags |= _lib.ZP_KCONST
    zt = ZpTerm(flags, 0 if zpa is None else int(zpa), 0 if zpb is None else int(zpb), K, row, col, bmap,
                a_batch, b_batch, M, N)
    return acc, zt


def weight_bt(b: DeviceArray):
    """Pre-transposed, K-padded int8 copy of a constant [K, N] weight and its
    column sums (used for every call instead of per-call transposes)."""
    K, N = b.shape[-2:]
    kp = (K + 15) // 16 * 16
    bt = DeviceArray(b.shape[:-2] + (N, kp), b.dtype)
    if kp != K:
        bt.fill_zero()
    bst = contiguous_strides(b.shape)
    copy_strided(b, bt, b.shape[:-2] + (N, K), list(bst[:-2]) + [bst[-1], bst[-2]],
                 contiguous_strides(b.shape[:-2] + (N, kp)))
    nb = int(math.prod(b.shape[:-2]))
    col = rowsum(bt, nb, N, kp, kp, N * kp)
    return bt, col


# ----------------------------------------------------------------------------- float GEMM
def sgemm(a: DeviceArray, a_sm, a_sk, b: DeviceArray, b_sk, b_sn, M, N, K, batch=1, bmap=None,
          a_ms=0, b_ms=0, transb=False) -> DeviceArray:
    """C = A[M, K] . B[K, N] per matrix in np.matmul's order for OpenBLAS at openblas_threads()
    threads (nqk_sgemm).  `transb`: B is, in the reference, the transposed view of a row-major
    [N, K] matrix (a Gemm's w.T, a Transpose node's output); it selects the small-matrix kernels'
    order and says nothing about the strides given here."""
    c = DeviceArray((batch, M, N) if batch > 1 else (M, N), np.float32)
    _lib.call("nqk_sgemm", a.vp, b.vp, c.vp, batch, M, N, K, a_sm, a_sk, b_sk, b_sn, N,
              _lib.i64arr(bmap) if bmap is not None else None, a_ms, b_ms, M * N, openblas_threads(),
              1 if transb else 0)
    return c


def blas_kblocks(K: int, threaded: bool) -> list:
    """OpenBLAS's level-3 K blocks (GEMM_Q = 448) under its threaded or its single-thread driver
    (nqk_gemm.hip blas_kblocks)."""
    out, ls = [], 0
    while ls < K:
        m = K - ls
        if m >= 896:
            m = 448
        elif m > 448:
            m = (m + 1) // 2 if threaded else ((m // 2 + 15) // 16) * 16
        out.append(m)
        ls += m
    return out


def gemm_small_regime(M: int, N: int, K: int, transb: bool = False) -> bool:
    """Whether np.matmul of A[M, K] @ B[K, N] (M, N >= 2) runs OpenBLAS's small-matrix kernels
    (SkylakeX permit: at most 100^3 multiply-adds; with B a transposed view only for M N <= 1200
    and K >= 32) instead of the level-3 drivers.  nqk_gemm.hip gemm_small_regime is the same rule."""
    if M * N * K > 1_000_000:
        return False
    return (not transb) or (M * N <= 1200 and K >= 32)


def gemm_restated(M: int, N: int, K: int, transb: bool = False) -> bool:
    """Whether A[M, K] @ B[K, N] with both operands contiguous (transb: B the transposed view of a
    contiguous [N, K]) is computed in np.matmul's exact order (tests/test_sgemm_ref_host.py pins
    the restatement, tests/_sgemm_ref.py, to np.matmul): both level-3 drivers' K blocks, and the
    small-matrix kernels of both forms, every row and column class — every shape with M, N >= 2.
    One-row and one-column products are the level-2 routines': one_row_restated.  Not covered by
    this predicate (open regime): an A that is a transposed view in the reference (Gemm's
    transA, a Transpose node feeding a MatMul's left operand) in the small regime."""
    return M >= 2 and N >= 2 and K >= 1


# OpenBLAS thread count of the NumPy whose GEMV order is reproduced (its column split
# depends on it, oracle/openblas_order.py): NQK_BLAS_THREADS, else what OpenBLAS itself
# reads (OPENBLAS_NUM_THREADS, GOTO_NUM_THREADS, OMP_NUM_THREADS, else the CPUs this
# process may run on), at most 64 (scipy-openblas MAX_THREADS)
BLAS_THREADS = None


def openblas_threads() -> int:
    if BLAS_THREADS is not None:
        return int(BLAS_THREADS)
    for v in ("NQK_BLAS_THREADS", "OPENBLAS_NUM_THREADS", "GOTO_NUM_THREADS", "OMP_NUM_THREADS"):
        s = os.environ.get(v, "").strip()
        if s.isdigit() and int(s) > 0:
            return min(int(s), 64)
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 64))


def gemv_t_applies(M: int, N: int, K: int) -> bool:
    """NumPy sends a one-row product x[1, K] @ B[K, N] (N > 1) whose B has unit stride
    along K to OpenBLAS GEMV-T; nqk_sgemv_t reproduces its order for every K (the regular
    kernels, and for K <= 8 the small-m kernels of each thread chunk of at most 16 384
    columns: oracle/openblas_order.py, pinned against np.matmul)."""
    return M == 1 and N > 1


def small_one_row(N: int, K: int) -> bool:
    """A one-row product with a 1 x 1 result: NumPy calls cblas_sdot (nqk_sgemv_small)."""
    return N == 1


def one_row_restated(N: int, K: int) -> bool:
    """Whether x[1, K] @ B[K, N] with B's columns contiguous (a Gemm's w.T) is computed in
    NumPy's exact order (pinned against np.matmul, tests/test_host.py): since round 6 every
    such product is — sdot at every length, GEMV-T's regular and small-m kernels at every K.
    (A one-row product against a row-major B — a MatMul's weight — is GEMV-N: nqk_sgemv_n.)"""
    return N >= 1 and K >= 1


def sgemv_small(x: DeviceArray, bt: DeviceArray) -> DeviceArray:
    """y[1, 1] = x[1, K] . bt[1, K]^T in cblas_sdot's order (nqk_sgemv_small)."""
    N, Kb = bt.shape
    K = x.shape[-1]
    if Kb != K or x.size != K:
        raise ValueError(f"matmul: mismatch in core dimension ({K} vs {Kb})")
    y = DeviceArray((1, N), np.float32)
    _lib.call("nqk_sgemv_small", x.vp, bt.vp, y.vp, N, K, K)
    return y


def sgemv_t(x: DeviceArray, bt: DeviceArray) -> DeviceArray:
    """y[1, N] = x[1, K] . bt[N, K]^T in OpenBLAS GEMV-T order (nqk_sgemv_t)."""
    N, Kb = bt.shape
    K = x.shape[-1]
    if Kb != K or x.size != K:
        raise ValueError(f"matmul: mismatch in core dimension ({K} vs {Kb})")
    y = DeviceArray((1, N), np.float32)
    _lib.call("nqk_sgemv_t", x.vp, bt.vp, y.vp, N, K, K, openblas_threads())
    return y


def matmul_f32(a: DeviceArray, b: DeviceArray, transb: bool = False) -> DeviceArray:
    """np.matmul for float32 (batched, broadcast), BLAS summation order.  `transb` as sgemm's
    (b is the materialised [.., K, N] either way)."""
    M, K = a.shape[-2:]
    K2, N = b.shape[-2:]
    if K != K2:
        raise ValueError(f"matmul: mismatch in core dimension ({K} vs {K2})")
    if (M == 1 or N == 1) and K > 1:
        return _matmul_level2(a, b, M, N, K)
    out_batch, bmap = batch_map(a.shape[:-2], b.shape[:-2])
    if bmap is None:
        a = materialize_broadcast(a, out_batch + (M, K))
        b = materialize_broadcast(b, out_batch + (K, N))
        _, bmap = batch_map(out_batch, out_batch)
    nb = int(math.prod(out_batch))
    c = sgemm(a, K, 1, b, N, 1, M, N, K, batch=nb, bmap=bmap, a_ms=M * K, b_ms=K * N, transb=transb)
    return c.reshape(out_batch + (M, N))


def _matmul_level2(a: DeviceArray, b: DeviceArray, M: int, N: int, K: int) -> DeviceArray:
    """np.matmul where one side of each product is a vector: NumPy's matmul (matmul.cpp special
    cases, per matrix of a stack) calls cblas_sdot for a 1 x 1 result, and cblas_sgemv for
    vector @ matrix — OpenBLAS GEMV-N on a row-major matrix (nqk_sgemv_n) — and for matrix @
    vector — GEMV-T over the matrix's rows (nqk_sgemv_t); each restated bit for bit
    (oracle/openblas_order.py, round 6).  (K = 1 stays on the GEMM path: NumPy's own loop, one
    product per output.)"""
    out_batch = tuple(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]))
    if a.shape[:-2] != out_batch:
        a = materialize_broadcast(a, out_batch + (M, K))
    if b.shape[:-2] != out_batch:
        b = materialize_broadcast(b, out_batch + (K, N))
    c = DeviceArray(out_batch + (M, N), np.float32)
    t = openblas_threads()
    for i in range(int(math.prod(out_batch))):
        ai, bi, ci = a.offset_view(i * M * K, (M, K)), b.offset_view(i * K * N, (K, N)), c.offset_view(i * M * N, (M, N))
        if M == 1 and N == 1:
            _lib.call("nqk_sgemv_small", ai.vp, bi.vp, ci.vp, 1, K, K)
        elif M == 1:
            _lib.call("nqk_sgemv_n", ai.vp, bi.vp, ci.vp, N, K, N, t)
        else:
            _lib.call("nqk_sgemv_t", bi.vp, ai.vp, ci.vp, M, K, K, t)
    return c


def sgemv_n(x: DeviceArray, b: DeviceArray) -> DeviceArray:
    """y[1, N] = x[1, K] . b[K, N] (b row-major) in OpenBLAS GEMV-N order (nqk_sgemv_n)."""
    K, N = b.shape
    if x.size != K:
        raise ValueError(f"matmul: mismatch in core dimension ({x.size} vs {K})")
    y = DeviceArray((1, N), np.float32)
    _lib.call("nqk_sgemv_n", x.vp, b.vp, y.vp, N, K, N, openblas_threads())
    return y


# ----------------------------------------------------------------------------- float ops
def binary(op: int, a: DeviceArray, b: DeviceArray) -> DeviceArray:
    out_shape = tuple(np.broadcast_shapes(a.shape, b.shape))
    out = DeviceArray(out_shape, np.float32)
    sa = broadcast_strides(a.shape, out_shape)
    sb = broadcast_strides(b.shape, out_shape)
    shp, (sa, sb) = collapse(out_shape, sa, sb)
    if len(shp) > 6:
        raise ValueError("elementwise op over more than 6 non-mergeable dimensions")
    _lib.call("nqk_binary_f32", op, a.vp, b.vp, out.vp, len(shp), _lib.i64arr(shp), _lib.i64arr(sa),
              _lib.i64arr(sb))
    return out


def unary(op: int, x: DeviceArray) -> DeviceArray:
    out = DeviceArray(x.shape, np.float32)
    _lib.call("nqk_unary_f32", op, x.vp, out.vp, x.size)
    return out


def add_scalar(x: DeviceArray, s: float) -> DeviceArray:
    out = DeviceArray(x.shape, np.float32)
    _lib.call("nqk_add_scalar_f32", x.vp, float(np.float32(s)), out.vp, x.size)
    return out


def _axis_split(x: DeviceArray, axis: int):
    """(outer, n, inner) of a contiguous array around `axis`.  NumPy sums an axis that still
    has elements after it (inner > 1) one term at a time in index order; only an effectively
    innermost axis (inner == 1: trailing extents of 1 dropped) gets pairwise summation."""
    if not -x.ndim <= axis < x.ndim:
        raise ValueError(f"axis {axis} is out of bounds for array of dimension {x.ndim}")
    axis %= x.ndim
    return int(math.prod(x.shape[:axis])), x.shape[axis], int(math.prod(x.shape[axis + 1:]))


# longest innermost axis of the pairwise row kernels (nqk_numerics.h: 64 leaves of 128)
MAX_ROW = 8192


def _check_row(cols: int) -> None:
    if cols > MAX_ROW:
        raise ValueError(f"reduction over an innermost axis of {cols} elements: the pairwise-sum plan "
                         f"covers at most {MAX_ROW}")


def softmax(x: DeviceArray, axis: int) -> DeviceArray:
    outer, n, inner = _axis_split(x, axis)
    out = DeviceArray(x.shape, np.float32)
    if x.size == 0:
        return out
    if inner == 1:
        _check_row(n)
        _lib.call("nqk_softmax_lastdim", x.vp, out.vp, outer, n)
    else:
        _lib.call("nqk_softmax_axis", x.vp, out.vp, outer, n, inner)
    return out


TOPK_MAX_K = 64       # one winner per lane of the row's wave (nqk_topk.hip)
TOPK_MAX_COLS = 8192  # the pairwise-sum plan's limit, as for the other row kernels


def topk_softmax(x: DeviceArray, k: int, scale=None, zp=None, prob: bool = True, value: bool = False):
    """Top-k of the last axis with the Softmax probabilities of the selected elements
    (nqk_topk_softmax): `(indices int64, probabilities | None, values | None)`, each a
    DeviceArray of shape x.shape[:-1] + (k,).

    x is float32 (scale and zp stay None) or the integer storage of a QTensor with its
    `scale` and scalar (or no) zero point; the integer form equals the float form on
    `dequantize(x, scale, zp)` without materialising it.  Per row,
    indices = np.argsort(-y, kind="stable")[:k] and probabilities are the bits `softmax(y, -1)`
    holds at those indices.  Every argument is checked here, before the library is touched."""
    if isinstance(zp, ZpTerm):
        raise ValueError("topk_softmax: a q_matmul zero-point term (ZpTerm) is not supported; requantize first")
    if zp is not None and np.ndim(zp):
        raise ValueError("topk_softmax: the zero point must be a scalar or None")
    if x.ndim < 1:
        raise ValueError("topk_softmax: the input needs at least one axis")
    if x.dtype == np.float32:
        if scale is not None or zp is not None:
            raise ValueError("topk_softmax: scale and zero point belong to integer input only")
    elif x.dtype.kind == "i" and x.dtype in (np.int8, np.int16, np.int32, np.int64):
        if scale is None:
            raise ValueError("topk_softmax: integer input needs its scale")
    else:
        raise ValueError(f"topk_softmax: dtype {x.dtype} not supported (float32 or int8 / int16 / int32 / int64)")
    cols = x.shape[-1]
    rows = int(math.prod(x.shape[:-1]))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"topk_softmax: k must be an integer, not {type(k).__name__}")
    k = int(k)
    if cols > TOPK_MAX_COLS:
        raise ValueError(f"topk_softmax: rows of {cols} elements (at most {TOPK_MAX_COLS})")
    if not 1 <= k <= min(cols, TOPK_MAX_K):
        raise ValueError(f"topk_softmax: k = {k} outside 1..min(cols = {cols}, {TOPK_MAX_K})")
    shape = x.shape[:-1] + (k,)
    idx = DeviceArray(shape, np.int64)
    p = DeviceArray(shape, np.float32) if prob else None
    v = DeviceArray(shape, np.float32) if value else None
    _lib.call("nqk_topk_softmax", x.vp, x.code, float(np.float32(1.0 if scale is None else scale)),
              0 if zp is None else int(zp), 0 if zp is None else 1, rows, cols, cols, k, idx.vp,
              p.vp if p is not None else None, v.vp if v is not None else None)
    return idx, p, v


def layernorm(x: DeviceArray, g: DeviceArray, b: DeviceArray, axis: int, eps: float) -> DeviceArray:
    """model.py:134-152.  Scale and bias broadcast against x as NumPy broadcasts them."""
    outer, n, inner = _axis_split(x, axis)
    axis %= x.ndim
    eps = float(np.float32(eps))
    out_shape = tuple(np.broadcast_shapes(x.shape, g.shape, b.shape))
    if x.size == 0:
        return DeviceArray(out_shape, np.float32)
    if inner > 1:
        norm = DeviceArray(x.shape, np.float32)
        _lib.call("nqk_normalize_axis", x.vp, norm.vp, outer, n, inner, eps)
        return binary(_lib.ADD, binary(_lib.MUL, norm, g), b)
    # innermost axis: the row kernel applies a scale and bias that vary along that axis alone
    _check_row(n)
    along = (1,) * axis + (n,) + (1,) * (x.ndim - 1 - axis)
    for t in (g, b):
        if t.size != 1 and (t.ndim > x.ndim or (1,) * (x.ndim - t.ndim) + t.shape != along):
            raise ValueError("LayerNormalization scale/bias must cover the normalised axis "
                             f"({t.shape} against {x.shape}, axis {axis})")
    if out_shape != x.shape:
        raise ValueError(f"LayerNormalization scale/bias of more dimensions than the input {x.shape}")
    if g.size != n:
        g = materialize_broadcast(g.reshape(()), (n,))
    if b.size != n:
        b = materialize_broadcast(b.reshape(()), (n,))
    out = DeviceArray(x.shape, np.float32)
    _lib.call("nqk_layernorm_lastdim", x.vp, g.vp, b.vp, out.vp, outer, n, eps)
    return out


def mean_axis(x: DeviceArray, axis: int, keepdims: bool) -> DeviceArray:
    """np.mean(x, axis, keepdims=keepdims) for float32 (tensor.py:127-128)."""
    outer, n, inner = _axis_split(x, axis)
    axis %= x.ndim
    shape = x.shape[:axis] + ((1,) if keepdims else ()) + x.shape[axis + 1:]
    if n == 0:
        raise ValueError("mean of an empty axis")
    out = DeviceArray(shape, np.float32)
    if out.size == 0:
        return out
    if inner == 1:
        _check_row(n)
        _lib.call("nqk_mean_lastdim", x.vp, out.vp, outer, n)
    else:
        _lib.call("nqk_mean_axis", x.vp, out.vp, outer, n, inner)
    return out


def minmax(x: DeviceArray) -> tuple[np.float32, np.float32]:
    scratch = DeviceArray((4096,), np.float32)
    res = DeviceArray((2,), np.float32)
    _lib.call("nqk_minmax_f32", x.vp, x.size, res.vp, scratch.vp, 4096)
    h = res.to_host()
    return h[0], h[1]


HIST_SHIFT = 18                  # NQK_HIST_SHIFT: bin = key >> 18 (sign, exponent, 5 mantissa bits)
HIST_BINS = 1 << (32 - HIST_SHIFT)  # NQK_HIST_BINS
HIST_MAX_N = 1 << 40             # NQK_HIST_MAX_N
# NQK_HIST_DIRECT_MAX: arrays up to this size are added straight into the state, longer ones
# through per-workgroup LDS histograms (nqk_hist.hip).  Measured with tools/bench_calibration.py
# (DESIGN.md §4.10): straight 3.6 us at 4 Ki elements, 5.0 at 8 Ki, 8.5 at 16 Ki and 15.6 at
# 32 Ki; through LDS 6.8-6.9 us at each of them.  They cross near 12 Ki.
HIST_DIRECT_MAX = 8192


def histogram(x: DeviceArray, state: DeviceArray, counts: bool = True) -> None:
    """Accumulate the key histogram and key range of float32 `x` into `state`, int64
    [HIST_BINS + 2] on the device (nqk_hist_f32; calibration.py states the layout).  Asynchronous;
    `counts=False` updates the two range entries only.  Everything is checked here, before the
    library is touched."""
    if not isinstance(x, DeviceArray) or not isinstance(state, DeviceArray):
        raise ValueError("histogram: x and state must be DeviceArrays")
    if x.dtype != np.float32:
        raise ValueError(f"histogram: x must be float32 (got {x.dtype})")
    if state.dtype != np.int64 or state.shape != (HIST_BINS + 2,):
        raise ValueError(f"histogram: state must be int64 [{HIST_BINS + 2}] (got {state.dtype} {state.shape})")
    if x.ptr % 4 or state.ptr % 8:
        raise ValueError("histogram: x needs 4-byte and state 8-byte alignment")
    if x.size > HIST_MAX_N:
        raise ValueError(f"histogram: more than {HIST_MAX_N} elements")
    for arr, what in ((x, "x"), (state, "state")):
        if arr.ptr < arr.block.ptr or arr.ptr + arr.nbytes > arr.block.ptr + arr.block.size:
            raise ValueError(f"histogram: {what} reaches outside its buffer")
    if x.size == 0:
        return
    _lib.call("nqk_hist_f32", x.vp, x.size, state.vp, 1 if counts else 0)


ABSMAX_NAN_KEY = 0x7FC00000  # the key of every NaN in an nqk_absmax_f32 state


def absmax(x: DeviceArray, state: DeviceArray, axis: int = 0, rows=None, cols=None, ld=None) -> None:
    """Accumulate the largest magnitude of every column (axis 0) or row (axis 1) of float32 `x`,
    read as [rows, ld] with `cols` columns used (default: a 2-D x as it lies), into `state`, uint32
    [cols] or [rows] on the device (nqk_absmax_f32: the state viewed as float32 is
    np.abs(x).max(axis)).  Asynchronous; everything is checked here, before the library is touched."""
    if not isinstance(x, DeviceArray) or not isinstance(state, DeviceArray):
        raise ValueError("absmax: x and state must be DeviceArrays")
    if x.dtype != np.float32 or state.dtype != np.uint32:
        raise ValueError(f"absmax: x must be float32 and state uint32 (got {x.dtype}, {state.dtype})")
    if axis not in (0, 1):
        raise ValueError(f"absmax: axis must be 0 or 1 (got {axis!r})")
    if rows is None:
        if x.ndim != 2:
            raise ValueError("absmax: give rows, cols and ld for an array that is not 2-D")
        rows, cols = x.shape
    rows, cols = int(rows), int(cols)
    ld = cols if ld is None else int(ld)
    if rows < 0 or cols < 0 or cols > ld:
        raise ValueError(f"absmax: bad sizes (rows {rows}, cols {cols}, ld {ld})")
    if state.shape != ((cols,) if axis == 0 else (rows,)):
        raise ValueError(f"absmax: state must be uint32 [{cols if axis == 0 else rows}] (got {state.shape})")
    if rows and cols and (rows - 1) * ld + cols > x.size:
        raise ValueError(f"absmax: [{rows}, {cols}] with ld {ld} reaches past the {x.size} elements of x")
    if x.ptr % 4 or state.ptr % 4:
        raise ValueError("absmax: x and state need 4-byte alignment")
    for arr, what in ((x, "x"), (state, "state")):
        if arr.ptr < arr.block.ptr or arr.ptr + arr.nbytes > arr.block.ptr + arr.block.size:
            raise ValueError(f"absmax: {what} reaches outside its buffer")
    if rows == 0 or cols == 0:
        return
    _lib.call("nqk_absmax_f32", x.vp, rows, cols, ld, axis, state.vp)


CMP_STATE = 8            # NQK_CMP_STATE: words of a comparison state
CMP_CHUNK = 4096         # NQK_CMP_CHUNK: elements per chunk partial
CMP_MAX_N = 1 << 36      # NQK_CMP_MAX_N


def compare_stats(x: DeviceArray, y: DeviceArray, state: DeviceArray, scale=None, zp=None) -> None:
    """Accumulate the error statistics of `y` against float32 `x` into `state`, int64 [CMP_STATE]
    on the device (nqk_compare_stats; compare.py states the layout and the order of the sums).
    y is float32 (scale and zp stay None) or the integer storage of a QTensor with its `scale`
    and scalar (or no) zero point, read as `dequantize(y, scale, zp)` without materialising it.
    Asynchronous.  Every argument is checked here, before the library is touched."""
    if isinstance(zp, ZpTerm):
        raise ValueError("compare_stats: a q_matmul zero-point term (ZpTerm) is not supported; dequantize first")
    if not all(isinstance(a, DeviceArray) for a in (x, y, state)):
        raise ValueError("compare_stats: x, y and state must be DeviceArrays")
    if zp is not None and np.ndim(zp):
        raise ValueError("compare_stats: the zero point must be a scalar or None")
    if x.dtype != np.float32:
        raise ValueError(f"compare_stats: x must be float32 (got {x.dtype})")
    if y.dtype == np.float32:
        if scale is not None or zp is not None:
            raise ValueError("compare_stats: scale and zero point belong to integer y only")
    elif y.dtype in (np.int8, np.int16, np.int32, np.int64):
        if scale is None:
            raise ValueError("compare_stats: integer y needs its scale")
    else:
        raise ValueError(f"compare_stats: dtype {y.dtype} not supported (float32 or int8 / int16 / int32 / int64)")
    if x.shape != y.shape:
        raise ValueError(f"compare_stats: shapes differ ({x.shape} against {y.shape})")
    if state.dtype != np.int64 or state.shape != (CMP_STATE,):
        raise ValueError(f"compare_stats: state must be int64 [{CMP_STATE}] (got {state.dtype} {state.shape})")
    if x.ptr % 4 or y.ptr % y.dtype.itemsize or state.ptr % 8:
        raise ValueError("compare_stats: x and y need the alignment of their elements, state 8 bytes")
    if x.size > CMP_MAX_N:
        raise ValueError(f"compare_stats: more than {CMP_MAX_N} elements")
    for arr, what in ((x, "x"), (y, "y"), (state, "state")):
        if arr.ptr < arr.block.ptr or arr.ptr + arr.nbytes > arr.block.ptr + arr.block.size:
            raise ValueError(f"compare_stats: {what} reaches outside its buffer")
    if x.size == 0:
        return
    chunks = (x.size + CMP_CHUNK - 1) // CMP_CHUNK
    scratch = DeviceArray((3 * chunks,), np.float64)
    _lib.call("nqk_compare_stats", x.vp, y.vp, _lib.NQK_F32 if y.dtype == np.float32 else y.code,
              float(np.float32(1.0 if scale is None else scale)), 0 if zp is None else int(zp),
              0 if zp is None else 1, x.size, state.vp, scratch.vp, 3 * chunks)


def where(cond: np.ndarray, a: DeviceArray, b: DeviceArray) -> DeviceArray:
    c = DeviceArray.from_host(np.asarray(cond).astype(np.int64))
    out_shape = tuple(np.broadcast_shapes(c.shape, a.shape, b.shape))
    out = DeviceArray(out_shape, np.float32)
    sc, sa, sb = (broadcast_strides(t.shape, out_shape) for t in (c, a, b))
    shp, (sc, sa, sb) = collapse(out_shape, sc, sa, sb)
    if len(shp) > 6:
        raise ValueError("elementwise op over more than 6 non-mergeable dimensions")
    _lib.call("nqk_where_f32", c.vp, a.vp, b.vp, out.vp, len(shp), _lib.i64arr(shp), _lib.i64arr(sc),
              _lib.i64arr(sa), _lib.i64arr(sb))
    return out


def im2col(x: DeviceArray, kh, kw, pads, strides):
    n, c, h, w = x.shape
    ph0, pw0, ph1, pw1 = pads
    sh, sw = strides
    ho = int(np.ceil((h - kh + ph0 + ph1 + 1) / sh))
    wo = int(np.ceil((w - kw + pw0 + pw1 + 1) / sw))
    cols = DeviceArray((n * ho * wo, kh * kw * c), np.float32)
    _lib.call("nqk_im2col", x.vp, cols.vp, n, c, h, w, kh, kw, ph0, pw0, sh, sw, ho, wo)
    return cols, ho, wo


# ----------------------------------------------------------------------------- integer Conv
def _inside(arr: DeviceArray) -> bool:
    return arr.ptr >= arr.block.ptr and arr.ptr + arr.nbytes <= arr.block.ptr + arr.block.size


def im2col_q(x: DeviceArray, kh, kw, pads, strides, pad: int = 0, rowsum: bool = False):
    """`im2col` of integer storage (nqk_im2col_q): `(cols, row sums | None, ho, wo)`, cols in x's
    dtype with padded cells = `pad` (the zero point); the int64 row sums are cols.sum(1).  Every
    argument is checked here, before the library is touched."""
    if not isinstance(x, DeviceArray) or x.ndim != 4:
        raise ValueError("im2col_q: a 4-d (NCHW) DeviceArray expected")
    if x.dtype not in (np.int8, np.int16, np.int32, np.int64):
        raise ValueError(f"im2col_q: dtype {x.dtype} not supported (int8 / int16 / int32 / int64)")
    n, c, h, w = x.shape
    kh, kw = int(kh), int(kw)
    ph0, pw0, ph1, pw1 = (int(p) for p in pads)
    sh, sw = (int(s) for s in strides)
    if kh < 1 or kw < 1 or sh < 1 or sw < 1 or min(ph0, pw0, ph1, pw1) < 0:
        raise ValueError("im2col_q: kernel and strides of at least 1 and non-negative pads expected")
    pad = int(pad)
    info = np.iinfo(x.dtype)
    if not info.min <= pad <= info.max:
        raise ValueError(f"im2col_q: the pad value {pad} does not fit {x.dtype}")
    ho = max(0, (h - kh + ph0 + ph1) // sh + 1)
    wo = max(0, (w - kw + pw0 + pw1) // sw + 1)
    if not _inside(x):
        raise ValueError("im2col_q: x reaches outside its buffer")
    cols = DeviceArray((n * ho * wo, kh * kw * c), x.dtype)
    rs = DeviceArray((n * ho * wo,), np.int64) if rowsum else None
    _lib.call("nqk_im2col_q", x.vp, cols.vp, x.code, rs.vp if rs is not None else None, n, c, h, w, kh, kw, ph0,
              pw0, sh, sw, ho, wo, pad)
    return cols, rs, ho, wo


EMBED_QI8_MAX_ZP = 1 << 20


def embed_qi8_fits(images: int, c: int, h: int, w: int, kh: int, kw: int, kout: int, zx) -> bool:
    """Whether nqk_embed_qi8 takes the shape (its own refusals, include/nqk.h)."""
    zx = 0 if zx is None else int(zx)
    kk = c * kh * kw
    return (kh == 16 and kw == 16 and h > 0 and w > 0 and h % 16 == 0 and w % 16 == 0 and kk % 64 == 0 and kout > 0 and
            kout % 64 == 0 and abs(zx) <= EMBED_QI8_MAX_ZP and kk * (1 << 14) + abs(zx) * kk * (1 << 7) < (1 << 31) and
            images <= 1 << 24 and kout <= 1 << 24 and h <= 1 << 20 and w <= 1 << 20 and
            -(-(images * (h // 16) * (w // 16)) // 128) * (kout // 64) <= 2147483647)


def embed_qi8(q: DeviceArray, wt: DeviceArray, colterm: DeviceArray, scale, zx, w_l1max: int, bias: DeviceArray,
              cls: DeviceArray, pos: DeviceArray, out: DeviceArray) -> None:
    """nqk_embed_qi8 (include/nqk.h) into `out` [images][hw + 1][N]: q int8 [images][c][h][w] in
    16 x 16 patches, wt int8 [N][c * 256] (the Conv weight as it lies), colterm int32 [N] =
    zx * wt.sum(1).  Every extent is checked here against its buffer, before the library is
    touched; the library checks alignment and the value ranges again."""
    for arr, what, dt in ((q, "q", np.int8), (wt, "wt", np.int8), (colterm, "colterm", np.int32),
                          (bias, "bias", np.float32), (cls, "cls", np.float32), (pos, "pos", np.float32),
                          (out, "out", np.float32)):
        if not isinstance(arr, DeviceArray) or arr.dtype != dt:
            raise ValueError(f"embed_qi8: {what} must be a {np.dtype(dt)} DeviceArray")
        if not _inside(arr):
            raise ValueError(f"embed_qi8: {what} reaches outside its buffer")
    if q.ndim != 4 or wt.ndim != 2:
        raise ValueError("embed_qi8: q [images][c][h][w] and wt [N][K] expected")
    n, c, h, w = q.shape
    kout, kk = wt.shape
    if kk != c * 256:
        raise ValueError(f"embed_qi8: wt has K = {kk}, the image needs {c * 256}")
    if not embed_qi8_fits(n, c, h, w, 16, 16, kout, zx):
        raise ValueError(f"embed_qi8: shape not taken (images {n}, c {c}, {h} x {w}, N {kout}, zero point {zx})")
    hw = (h // 16) * (w // 16)
    if colterm.size != kout or bias.size != kout or cls.size != kout or pos.size != (hw + 1) * kout or \
            out.size != n * (hw + 1) * kout:
        raise ValueError("embed_qi8: colterm / bias / cls [N], pos [hw + 1][N] and out [images][hw + 1][N] expected")
    _lib.call("nqk_embed_qi8", q.vp, wt.vp, colterm.vp, float(np.float32(scale)), 0 if zx is None else int(zx),
              int(w_l1max), bias.vp, cls.vp, pos.vp, out.vp, n, c, h, w, 16, 16, kout)
