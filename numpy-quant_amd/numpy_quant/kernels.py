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


CLIP_MAX_G = 64  # candidates of one nqk_clip_search_cols call


def clip_ratios(steps: int) -> np.ndarray:
    """float32 [steps]: ratio[g] = f32(1 - 0.5 g / steps), the factor in float64; ratio[0] = 1."""
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= CLIP_MAX_G:
        raise ValueError(f"clip_steps must be an integer in 1..{CLIP_MAX_G} (got {steps!r})")
    return (1.0 - 0.5 * np.arange(int(steps), dtype=np.float64) / float(steps)).astype(np.float32)


def clip_search_cols(x: DeviceArray, s0, ratios, bit_width: int, want_err: bool = False, rows=None, cols=None,
                     ld=None):
    """The clipping search of every column of float32 `x`, read as [rows, ld] with `cols` columns used
    (default: a 2-D x as it lies): for column n and candidate g the float64 squared error of
    quantize_cols / dequantize_cols at `bit_width` with the scale f32(s0[n] * ratios[g]), in the
    fixed order include/nqk.h states (nqk_clip_search_cols).  `s0` float32 [cols] and `ratios`
    float32 [G], 1 <= G <= 64, on the host or the device.  Returns (scale float32 [cols], index
    int32 [cols]) on the device: the first candidate with the smallest error and its scale; with
    `want_err` also err float64 [G, cols].  A column whose s0 is 0 or not finite comes back as it
    is, with index 0.  Asynchronous; everything is checked here, before the library is touched."""
    if not isinstance(x, DeviceArray) or x.dtype != np.float32:
        raise ValueError("clip_search_cols: x must be a float32 DeviceArray")
    if rows is None:
        if x.ndim != 2:
            raise ValueError("clip_search_cols: give rows, cols and ld for an array that is not 2-D")
        rows, cols = x.shape
    rows, cols = int(rows), int(cols)
    ld = cols if ld is None else int(ld)
    if rows < 1 or cols < 1 or cols > ld:
        raise ValueError(f"clip_search_cols: bad sizes (rows {rows}, cols {cols}, ld {ld})")
    if (rows - 1) * ld + cols > x.size:
        raise ValueError(f"clip_search_cols: [{rows}, {cols}] with ld {ld} reaches past the {x.size} elements of x")
    if x.ptr % 4 or x.ptr < x.block.ptr or x.ptr + x.nbytes > x.block.ptr + x.block.size:
        raise ValueError("clip_search_cols: x is misaligned or reaches outside its buffer")
    if isinstance(bit_width, bool) or not isinstance(bit_width, (int, np.integer)) or not 1 <= bit_width <= 8:
        raise ValueError(f"clip_search_cols: bit_width must be an integer in 1..8 (got {bit_width!r})")
    vecs = []
    for v, what, n in ((s0, "s0", cols), (ratios, "ratios", None)):
        if not isinstance(v, DeviceArray):
            v = np.asarray(v)
            if v.dtype != np.float32:
                raise ValueError(f"clip_search_cols: {what} must be float32 (got {v.dtype})")
            v = DeviceArray.from_host(v)
        if v.dtype != np.float32 or v.ndim != 1 or (n is not None and v.shape != (n,)):
            raise ValueError(f"clip_search_cols: {what} must be a float32 vector" + (f" [{n}]" if n else ""))
        vecs.append(v)
    s0, ratios = vecs
    G = ratios.shape[0]
    if not 1 <= G <= CLIP_MAX_G:
        raise ValueError(f"clip_search_cols: 1..{CLIP_MAX_G} candidates (got {G})")
    scale, index = DeviceArray((cols,), np.float32), DeviceArray((cols,), np.int32)
    err = DeviceArray((G, cols), np.float64) if want_err else None
    _lib.call("nqk_clip_search_cols", x.vp, rows, cols, ld, s0.vp, ratios.vp, G, int(bit_width), scale.vp, index.vp,
              err.vp if want_err else None)
    return (scale, index, err) if want_err else (scale, index)


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
# nqk_qgemm_i16 (int16 activations as two byte planes on the int8 MFMAs): its shared cross-plane
# accumulator holds up to 2^15 per product, so the padded K stays below 2^16.  NQK_GEMM16=0 keeps
# such products on nqk_qgemm_generic (the A/B leg; read at every call).
I16_MAX_K = 1 << 16


def _gemm16_enabled() -> bool:
    return os.environ.get("NQK_GEMM16", "1") != "0"


def _gemm16_epi_enabled() -> bool:
    """NQK_GEMM16_EPI=1 opts in to nqk_qgemm_i16_epi; unset or 0 keeps nqk_qgemm_i16 and a separate
    dequantize / requantize launch (the A/B leg; read at every call).  Opt-in because one of the four
    model-level ranges of profiles/gemm16_epi.json overlaps."""
    return os.environ.get("NQK_GEMM16_EPI", "0") != "0"


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


class PendingProduct:
    """A q_matmul product on the int16 MFMA route that has not been launched: the padded operands of
    nqk_qgemm_i16 and, once `qmatmul` has it, the ZpTerm.  Its one consumer decides the launch:
    `materialize` is nqk_qgemm_i16 (the int64 array), `dequantize` and `requantize` are
    nqk_qgemm_i16_epi, which never writes that array.  All three are timed as "qgemm_i16"."""

    dtype = np.dtype(np.int64)

    def __init__(self, ap: DeviceArray, bt: DeviceArray, out_batch, M: int, N: int, K: int, kp: int, bmap):
        self.ap, self.bt, self.bmap = ap, bt, bmap
        self.shape = tuple(out_batch) + (M, N)
        self.nb, self.M, self.N, self.K, self.kp = int(math.prod(out_batch)), M, N, K, kp
        self.zp: ZpTerm | None = None

    @property
    def ndim(self) -> int:
        return len(self.shape)

    def _timed(self, out_bytes: int, name: str, *args):
        t0 = TIMER.begin() if TIMER is not None else None
        _lib.call(name, *args)
        if t0 is not None:  # one int8 MFMA product per pair of byte planes: 2 (int8 B) or 4
            nb, M, N, K, wb = self.nb, self.M, self.N, self.K, self.bt.dtype.itemsize
            TIMER.end("qgemm_i16", t0, (2 * nb * M * N * K * 2 * wb, nb * (2 * M * K + wb * N * K + out_bytes * M * N)))

    def materialize(self) -> DeviceArray:
        acc = DeviceArray(self.shape, np.int64)
        M, N, kp = self.M, self.N, self.kp
        self._timed(8, "nqk_qgemm_i16", self.ap.vp, self.bt.vp, self.bt.code, acc.vp, self.nb, M, N, kp, kp, kp, N,
                    _lib.i64arr(self.bmap), M * kp, N * kp, M * N)
        return acc

    def _epilogue(self, out: DeviceArray, scale, **fields) -> None:
        z = self.zp
        e = _lib.Gemm16Epilogue(**fields)
        if isinstance(scale, DeviceArray):
            _check_cols(scale, self.N, "nqk_qgemm_i16_epi")
            e.s_col = scale.ptr
        else:
            e.scale = float(np.float32(scale))
        if z is not None:
            e.zp_flags, e.zpa, e.zpb, e.zp_K = z.flags, z.zpa, z.zpb, z.K
            e.row = z.row.ptr if z.row is not None else None
            e.col = z.col.ptr if z.col is not None else None
        M, N, kp = self.M, self.N, self.kp
        self._timed(out.dtype.itemsize, "nqk_qgemm_i16_epi", self.ap.vp, self.bt.vp, self.bt.code, out.vp,
                    _lib.NQK_F32 if out.dtype == np.float32 else out.code, self.nb, M, N, kp, kp, kp, N,
                    _lib.i64arr(self.bmap), M * kp, N * kp, M * N, ctypes.byref(e))

    def dequantize(self, scale) -> DeviceArray:
        """`dequantize(self.materialize(), scale, self.zp)`, or `dequantize_cols` of a DeviceArray scale."""
        out = DeviceArray(self.shape, np.float32)
        self._epilogue(out, scale)
        return out

    def requantize(self, scale, bias: DeviceArray | None, res_scale, res_zp, bit_width: int) -> DeviceArray:
        """`requantize(self.materialize(), scale, self.zp, bias, ...)` (`requantize_cols` of a DeviceArray
        scale) at a bit width of 9..16, whose storage is int16."""
        if not 9 <= bit_width <= 16:
            raise ValueError(f"PendingProduct.requantize: bit width 9..16 (got {bit_width})")
        if bias is not None and bias.size != self.N:
            raise ValueError(f"bias of {bias.size} elements cannot broadcast over rows of {self.N}")
        out = DeviceArray(self.shape, np.int16)
        self._epilogue(out, scale, bias=bias.ptr if bias is not None else None,
                       bias_dtype=bias.code if bias is not None else _lib.NQK_I64,
                       res_scale=float(np.float32(res_scale)), res_zp=0 if res_zp is None else int(res_zp),
                       has_res_zp=0 if res_zp is None else 1, bit_width=int(bit_width))
        return out


def _pad_k(x: DeviceArray, rows_shape, k: int, kp: int) -> DeviceArray:
    """Copy [..., rows, k] into a zero-filled [..., rows, kp] (kp % 16 == 0)."""
    out = DeviceArray(tuple(rows_shape) + (kp,), x.dtype).fill_zero()
    shape = tuple(rows_shape) + (k,)
    copy_strided(x, out, shape, contiguous_strides(shape), contiguous_strides(tuple(rows_shape) + (kp,)))
    return out


def qmatmul(a: DeviceArray, b: DeviceArray, zpa, zpb, b_transposed: DeviceArray | None = None,
            b_colsum: DeviceArray | None = None, defer: bool = False):
    """q_matmul (numpy_quantization.py:44-61): returns (acc, ZpTerm | None).

    a: [..., M, K] and b: [..., K, N] integer DeviceArrays (contiguous).  The int8
    path needs Bt[..., N, Kp]; `b_transposed` (and its column sums) may be passed in
    pre-computed for constant weights.  With `defer`, a product of the int16 MFMA route comes
    back as a PendingProduct (with NQK_GEMM16_EPI=1 only): the caller launches it with its consumer.
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
    kp = (K + 15) // 16 * 16
    use_i8 = (a.dtype == np.int8 and b.dtype == np.int8 and M * N * K >= MFMA_MIN_WORK and nb <= 65535
              and K < I8_MAX_K)
    use_i16 = (a.dtype == np.int16 and b.dtype in (np.int8, np.int16) and M * N * K >= MFMA_MIN_WORK
               and nb <= 65535 and kp < I16_MAX_K and _gemm16_enabled())
    use_mfma = use_i8 or use_i16
    if use_mfma:
        ap = a if K == kp else _pad_k(a, a.shape[:-1], K, kp)
        if b_transposed is None:
            bt = DeviceArray(b_batch + (N, kp), b.dtype)
            if K != kp:
                bt.fill_zero()
            shape = b_batch + (N, K)
            bst = contiguous_strides(b.shape)
            src_st = list(bst[:-2]) + [bst[-1], bst[-2]]
            copy_strided(b, bt, shape, src_st, contiguous_strides(b_batch + (N, kp)))
        else:
            bt = b_transposed
        if use_i8:
            t0 = TIMER.begin() if TIMER is not None else None
            acc = DeviceArray(out_batch + (M, N), np.int32)
            _lib.call("nqk_qgemm_i8", ap.vp, bt.vp, acc.vp, nb, M, N, kp, kp, kp, N, _lib.i64arr(bmap),
                      M * kp, N * kp, M * N)
            if t0 is not None:
                TIMER.end("qgemm_i8", t0, (2 * nb * M * N * K, nb * (M * K + N * K + 4 * M * N)))
        else:
            acc = PendingProduct(ap, bt, out_batch, M, N, K, kp, bmap)
            if not (defer and _gemm16_epi_enabled()):
                acc = acc.materialize()
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
    if isinstance(acc, PendingProduct):
        acc.zp = zt
    return acc, zt


def weight_bt(b: DeviceArray):
    """Pre-transposed, K-padded copy of a constant int8 or int16 [K, N] weight and its
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


# ----------------------------------------------------------------------------- group-wise weight scales
def check_group_size(group_size) -> int:
    """`group_size` as an int: a positive multiple of 32, at most 16384 (nqk_qgemm_group's range)."""
    if (isinstance(group_size, bool) or not isinstance(group_size, (int, np.integer)) or group_size < 32
            or group_size % 32 or group_size > 16384):
        raise ValueError(f"group_size must be a positive multiple of 32, at most 16384 (got {group_size!r})")
    return int(group_size)


def group_colsum(bt: DeviceArray, g: int) -> DeviceArray:
    """int32 [K / g, N]: the sums of int8 `bt` [N, K] (weight_bt's image) over every group of g
    consecutive k (nqk_group_colsum); once per constant weight."""
    g = check_group_size(g)
    if bt.dtype != np.int8 or bt.ndim != 2 or bt.shape[1] % g:
        raise ValueError(f"group_colsum: int8 [N, K] with K a multiple of {g} expected (got {bt.dtype} {bt.shape})")
    N, K = bt.shape
    gsum = DeviceArray((K // g, N), np.int32)
    _lib.call("nqk_group_colsum", bt.vp, N, K, K, g, gsum.vp)
    return gsum


def qmatmul_group(a: DeviceArray, bt: DeviceArray, gsum: DeviceArray | None, sg: DeviceArray, zpa, g: int) -> DeviceArray:
    """float32 [..., M, N] of int8 `a` [..., M, K] times the grouped weight `bt` [N, K] (nqk_qgemm_group,
    include/nqk.h: the arithmetic): `sg` float32 [K / g, N] the products f32(s_a * S), `gsum` the
    weight's group_colsum (needed with a zero point `zpa`; None without).  The batch axes of `a` are
    folded into M.  Timed as "qgemm_group"."""
    g = check_group_size(g)
    if a.dtype != np.int8 or bt.dtype != np.int8 or a.ndim < 2 or bt.ndim != 2:
        raise ValueError("qmatmul_group: int8 a [..., M, K] and int8 bt [N, K] expected")
    N, K = bt.shape
    if a.shape[-1] != K or K % g:
        raise ValueError(f"qmatmul_group: K of a ({a.shape[-1]}) and of bt ({K}) must agree and be a multiple of {g}")
    G = K // g
    if sg.dtype != np.float32 or sg.shape != (G, N):
        raise ValueError(f"qmatmul_group: sg must be float32 [{G}, {N}]")
    if zpa is not None and (gsum is None or gsum.dtype != np.int32 or gsum.shape != (G, N)):
        raise ValueError(f"qmatmul_group: a zero point needs gsum, int32 [{G}, {N}]")
    M = a.size // K
    out = DeviceArray(a.shape[:-1] + (N,), np.float32)
    t0 = TIMER.begin() if TIMER is not None else None
    _lib.call("nqk_qgemm_group", a.vp, bt.vp, sg.vp, gsum.vp if zpa is not None else None, out.vp, M, N, K, K, K, N, g,
              0 if zpa is None else int(zpa), 0 if zpa is None else 1)
    if t0 is not None:
        TIMER.end("qgemm_group", t0, (2 * M * N * K, M * K + N * K + 4 * M * N + (4 if zpa is None else 8) * G * N))
    return out


class GroupProduct:
    """A product with a group-wise scaled weight that has not been launched: the operands of
    nqk_qgemm_group.  PendingProduct's counterpart, with one consumer: `dequantize`.  No integer
    accumulator exists for it, since every group's partial sum is rescaled inside the k loop."""

    def __init__(self, a: DeviceArray, bt: DeviceArray, gsum: DeviceArray, sg: DeviceArray, zpa, g: int):
        self.a, self.bt, self.gsum, self.sg, self.zpa, self.g = a, bt, gsum, sg, zpa, g
        self.shape = tuple(a.shape[:-1]) + (bt.shape[0],)

    @property
    def ndim(self) -> int:
        return len(self.shape)

    def dequantize(self) -> DeviceArray:
        return qmatmul_group(self.a, self.bt, self.gsum, self.sg, self.zpa, self.g)


# ----------------------------------------------------------------------------- per-token activation scales
ROWS_MAX_K = 1 << 16  # nqk_qgemm_rows: |P - z colsum| <= 255 * 128 * K must fit int32


class RowQuantized:
    """A float tensor [..., cols] quantized row by row (nqk_quantize_rows): `q` int8 [rows, ldq] with
    ldq = cols rounded up to 16 and zero pad bytes, `s` float32 [rows] and `z` int32 [rows] the rows'
    own scales and zero points.  The left operand of nqk_qgemm_rows; nothing else reads it."""

    def __init__(self, q: DeviceArray, s: DeviceArray, z: DeviceArray, shape, bit_width: int):
        self.q, self.s, self.z, self.shape, self.bit_width = q, s, z, tuple(shape), bit_width

    @property
    def ndim(self) -> int:
        return len(self.shape)


def quantize_rows(x: DeviceArray, bit_width: int) -> RowQuantized:
    """Every row of float32 `x` [..., cols] quantized with the asymmetric parameters of its own range
    clamped to include 0 (include/nqk.h: the arithmetic), in one read of `x`.  Timed as "quantize_rows"."""
    if not isinstance(x, DeviceArray) or x.dtype != np.float32 or x.ndim < 1 or x.size == 0:
        raise ValueError("quantize_rows expects a non-empty float32 DeviceArray of at least one dimension")
    if isinstance(bit_width, bool) or not isinstance(bit_width, (int, np.integer)) or not 2 <= bit_width <= 8:
        raise ValueError(f"quantize_rows: bit_width must be an integer in 2..8 (got {bit_width!r})")
    cols = x.shape[-1]
    rows = x.size // cols
    ldq = (cols + 15) // 16 * 16
    q, s, z = DeviceArray((rows, ldq), np.int8), DeviceArray((rows,), np.float32), DeviceArray((rows,), np.int32)
    t0 = TIMER.begin() if TIMER is not None else None
    _lib.call("nqk_quantize_rows", x.vp, q.vp, s.vp, z.vp, rows, cols, cols, ldq, int(bit_width))
    if t0 is not None:
        TIMER.end("quantize_rows", t0, (0, 4 * rows * cols + rows * ldq + 8 * rows))
    return RowQuantized(q, s, z, x.shape, int(bit_width))


def qmatmul_rows(a: RowQuantized, bt: DeviceArray, colsum: DeviceArray, sw: DeviceArray) -> DeviceArray:
    """float32 [..., N] of the row-quantized `a` [..., K] times the symmetric weight `bt` [N, Kp]
    (weight_bt's image, with its int64 `colsum` [N]) whose column scales are `sw` float32 [N]
    (nqk_qgemm_rows, include/nqk.h: the arithmetic).  Timed as "qgemm_rows"."""
    if not isinstance(a, RowQuantized) or bt.dtype != np.int8 or bt.ndim != 2:
        raise ValueError("qmatmul_rows: a RowQuantized operand and an int8 bt [N, K] expected")
    N, kp = bt.shape
    M = a.q.shape[0]
    if a.q.shape[1] != kp or (a.shape[-1] + 15) // 16 * 16 != kp:
        raise ValueError(f"qmatmul_rows: K of a ({a.shape[-1]}) does not pad to the K of bt ({kp})")
    if kp >= ROWS_MAX_K:
        raise ValueError(f"qmatmul_rows: K must stay below {ROWS_MAX_K} (got {kp})")
    _check_cols(sw, N, "qmatmul_rows")
    if colsum.dtype != np.int64 or colsum.size != N:
        raise ValueError(f"qmatmul_rows: colsum must be int64 [{N}]")
    out = DeviceArray(a.shape[:-1] + (N,), np.float32)
    t0 = TIMER.begin() if TIMER is not None else None
    _lib.call("nqk_qgemm_rows", a.q.vp, bt.vp, a.s.vp, a.z.vp, sw.vp, colsum.vp, out.vp, M, N, kp, kp, kp, N)
    if t0 is not None:
        TIMER.end("qgemm_rows", t0, (2 * M * N * kp, M * kp + N * kp + 4 * M * N + 8 * M + 12 * N))
    return out


class RowProduct:
    """A product of a row-quantized activation with a weight that has not been launched: the operands
    of nqk_qgemm_rows.  GroupProduct's counterpart, with one consumer: `dequantize`.  No integer
    accumulator exists for it, since the rank-one scale s[m] * sw[n] is applied in the GEMM's epilogue."""

    def __init__(self, a: RowQuantized, bt: DeviceArray, colsum: DeviceArray, sw: DeviceArray):
        self.a, self.bt, self.colsum, self.sw = a, bt, colsum, sw
        self.shape = tuple(a.shape[:-1]) + (bt.shape[0],)

    @property
    def ndim(self) -> int:
        return len(self.shape)

    def dequantize(self) -> DeviceArray:
        return qmatmul_rows(self.a, self.bt, self.colsum, self.sw)


# ----------------------------------------------------------------------------- microscaling (MX) operands
MX_FORMATS = {"mxfp8": 8, "mxfp4": 4}  # name -> bits per element, which is also the C ABI's format code
MX_PAIRS = (("mxfp8", "mxfp8"), ("mxfp8", "mxfp4"), ("mxfp4", "mxfp4"))  # (activation, weight) as nqk_gemm_mx takes them


def check_mx_format(fmt, what="mx format") -> str:
    if not isinstance(fmt, str) or fmt not in MX_FORMATS:
        raise ValueError(f"{what} must be one of {sorted(MX_FORMATS)} (got {fmt!r})")
    return fmt


class MxQuantized:
    """A float tensor [..., cols] in an MX format (nqk_quantize_mx): `q` uint8 [rows, ldq * bits / 8]
    with ldq = cols rounded up to 128 and zero elements in the padding, `scales` uint8 [rows, ldq / 32],
    one E8M0 byte per block of 32 consecutive columns.  An operand of nqk_gemm_mx; nothing else reads it."""

    def __init__(self, q: DeviceArray, scales: DeviceArray, fmt: str, shape):
        self.q, self.scales, self.format, self.shape = q, scales, check_mx_format(fmt), tuple(shape)
        bits = MX_FORMATS[fmt]
        ldq = scales.shape[-1] * 32
        if (q.dtype != np.uint8 or scales.dtype != np.uint8 or q.ndim != 2 or scales.ndim != 2 or ldq % 128
                or ldq < self.shape[-1] or q.shape != (scales.shape[0], ldq * bits // 8)):
            raise ValueError(f"MxQuantized: uint8 elements [rows, ldq * {bits} / 8] and scale bytes [rows, ldq / 32] with "
                             f"ldq a multiple of 128 expected (got {q.shape}, {scales.shape})")
        self.ldq = ldq

    @property
    def ndim(self) -> int:
        return len(self.shape)


def quantize_mx(x: DeviceArray, fmt: str) -> MxQuantized:
    """float32 `x` [..., cols], cols a multiple of 32, in the MX format `fmt`: every block of 32
    consecutive columns takes the power-of-two scale of its own largest magnitude (include/nqk.h: the
    rule), in one read of `x`.  Timed as "quantize_mx"."""
    if not isinstance(x, DeviceArray) or x.dtype != np.float32 or x.ndim < 1 or x.size == 0:
        raise ValueError("quantize_mx expects a non-empty float32 DeviceArray of at least one dimension")
    bits = MX_FORMATS[check_mx_format(fmt)]
    cols = x.shape[-1]
    if cols % 32:
        raise ValueError(f"quantize_mx: the last axis must be a multiple of 32 (got {cols})")
    rows = x.size // cols
    ldq = (cols + 127) // 128 * 128
    q, s = DeviceArray((rows, ldq * bits // 8), np.uint8), DeviceArray((rows, ldq // 32), np.uint8)
    t0 = TIMER.begin() if TIMER is not None else None
    _lib.call("nqk_quantize_mx", x.vp, q.vp, s.vp, rows, cols, cols, ldq, bits)
    if t0 is not None:
        TIMER.end("quantize_mx", t0, (0, 4 * rows * cols + q.nbytes + s.nbytes))
    return MxQuantized(q, s, fmt, x.shape)


def gemm_mx(a: MxQuantized, b: MxQuantized) -> DeviceArray:
    """float32 [..., N] of the MX operand `a` [..., K] times the MX weight `b`, held transposed [N, K]
    (nqk_gemm_mx, include/nqk.h: the arithmetic).  Timed as "gemm_mx"."""
    if not isinstance(a, MxQuantized) or not isinstance(b, MxQuantized) or b.ndim != 2:
        raise ValueError("gemm_mx: an MxQuantized activation and a 2-D MxQuantized weight [N, K] expected")
    if (a.format, b.format) not in MX_PAIRS:
        raise ValueError(f"gemm_mx: the format pair {(a.format, b.format)} is not one of {MX_PAIRS}")
    N, K = b.shape
    if a.shape[-1] != K:
        raise ValueError(f"gemm_mx: mismatch in core dimension ({a.shape[-1]} vs {K})")
    M = a.q.shape[0]
    out = DeviceArray(a.shape[:-1] + (N,), np.float32)
    t0 = TIMER.begin() if TIMER is not None else None
    _lib.call("nqk_gemm_mx", a.q.vp, a.scales.vp, MX_FORMATS[a.format], b.q.vp, b.scales.vp, MX_FORMATS[b.format],
              out.vp, M, N, K, a.ldq, b.ldq, N)
    if t0 is not None:
        TIMER.end("gemm_mx", t0, (2 * M * N * K, a.q.nbytes + b.q.nbytes + a.scales.nbytes + b.scales.nbytes + 4 * M * N))
    return out


class MxProduct:
    """A product of two MX operands that has not been launched: RowProduct's counterpart, with one
    consumer, `dequantize`.  The block scales are applied inside the matrix instruction."""

    def __init__(self, a: MxQuantized, b: MxQuantized):
        self.a, self.b = a, b
        self.shape = tuple(a.shape[:-1]) + (b.shape[0],)

    @property
    def ndim(self) -> int:
        return len(self.shape)

    def dequantize(self) -> DeviceArray:
        return gemm_mx(self.a, self.b)


# products that only dequantize() reads, and operands that only matmul reads: a QTensor on one of
# these has no integer array (`dev`)
FLOAT_PRODUCTS = (GroupProduct, RowProduct, MxProduct)
NO_ACCUMULATOR = FLOAT_PRODUCTS + (RowQuantized, MxQuantized)


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
