"""uint8 images as model inputs: per-channel normalize, layout change to NCHW and (for a
QModel) quantize, all as one table lookup on the device (nqk_image_lut).

`ImagePreprocess.reference` is the definition, in float32 NumPy.  Normalize and quantize
are elementwise per channel, so a uint8 pixel of channel c maps to one of 256 values:
`table()` holds the normalized ones, and `K.quantize(table, ...)` the quantized ones.  The
kernel gathers from the table and does no floating-point arithmetic, so its output is
`reference(img)` (or `quantize(reference(img))`) bit for bit.  The uint8 batch is a quarter
of the float32 one on the host link.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import kernels as K
from .device import DeviceArray
from .tensor import FTensor

_LAYOUTS = {"NHWC": _lib.IMG_NHWC, "NCHW": _lib.IMG_NCHW}


class ImagePreprocess:
    """`ImagePreprocess(mean, std, layout="NHWC", rescale=255)`: per-channel (1 to 4
    channels) `((img / rescale) - mean) / std` of uint8 images given in `layout`."""

    def __init__(self, mean, std, layout: str = "NHWC", rescale=255):
        self.mean = np.atleast_1d(np.asarray(mean, dtype=np.float32))
        self.std = np.atleast_1d(np.asarray(std, dtype=np.float32))
        if self.mean.ndim != 1 or self.mean.shape != self.std.shape or not 1 <= self.mean.size <= 4:
            raise ValueError("ImagePreprocess: mean and std are per channel, 1 to 4 channels")
        if not np.all(np.isfinite(self.mean)):
            raise ValueError("ImagePreprocess: mean must be finite")
        if not np.all(np.isfinite(self.std)) or np.any(self.std == 0):
            raise ValueError("ImagePreprocess: std must be nonzero and finite")
        if layout not in _LAYOUTS:
            raise ValueError(f"ImagePreprocess: layout {layout!r} is neither 'NHWC' nor 'NCHW'")
        self.rescale = np.float32(rescale)
        if not np.isfinite(self.rescale) or self.rescale == 0:
            raise ValueError("ImagePreprocess: rescale must be nonzero and finite")
        self.layout = layout
        self._table_dev = None

    def __repr__(self):
        return (f"ImagePreprocess(mean={self.mean.tolist()}, std={self.std.tolist()}, layout={self.layout!r}, "
                f"rescale={float(self.rescale)})")

    @property
    def channels(self) -> int:
        return int(self.mean.size)

    def key(self) -> tuple:
        """The values a lookup table depends on (read on every call: the arrays are mutable)."""
        return (self.mean.tobytes(), self.std.tobytes(), self.rescale.tobytes())

    # ------------------------------------------------------------------ host definition
    def check(self, images) -> tuple[int, int, int, int]:
        """ValueError unless `images` is a non-empty 4-d uint8 batch of this channel count;
        returns (n, c, h, w)."""
        if not isinstance(images, np.ndarray) or images.dtype != np.uint8:
            raise ValueError(f"ImagePreprocess: uint8 images expected, got {getattr(images, 'dtype', type(images))}")
        if images.ndim != 4:
            raise ValueError(f"ImagePreprocess: 4-d {self.layout} images expected, got shape {images.shape}")
        if self.layout == "NHWC":
            n, h, w, c = images.shape
        else:
            n, c, h, w = images.shape
        if c != self.channels:
            raise ValueError(f"ImagePreprocess: {c} channels in images of shape {images.shape} ({self.layout}), "
                             f"{self.channels} in mean / std")
        if n == 0 or h == 0 or w == 0:
            raise ValueError(f"ImagePreprocess: empty batch of shape {images.shape}")
        return n, c, h, w

    def reference(self, images: np.ndarray) -> np.ndarray:
        """The definition: float32 NCHW, float32 NumPy operations only."""
        self.check(images)
        bshape = (1, 1, 1, -1) if self.layout == "NHWC" else (1, -1, 1, 1)
        x = images.astype(np.float32) / self.rescale
        x = (x - self.mean.reshape(bshape)) / self.std.reshape(bshape)
        if self.layout == "NHWC":
            x = x.transpose(0, 3, 1, 2)
        return np.ascontiguousarray(x)

    def table(self) -> np.ndarray:
        """float32 [C, 256]: `reference` of the values 0..255 in each channel."""
        v = np.arange(256, dtype=np.uint8)
        shape = (1, 1, 256, self.channels) if self.layout == "NHWC" else (1, self.channels, 1, 256)
        img = np.broadcast_to(v.reshape((1, 1, 256, 1) if self.layout == "NHWC" else (1, 1, 1, 256)), shape)
        return np.ascontiguousarray(self.reference(np.ascontiguousarray(img)).reshape(self.channels, 256))

    # ------------------------------------------------------------------ device
    def table_device(self) -> DeviceArray:
        """`table()` on the device, rebuilt when mean / std / rescale changed."""
        key = self.key()
        if self._table_dev is None or self._table_dev[0] != key:
            self._table_dev = (key, DeviceArray.from_host(self.table()))
        return self._table_dev[1]

    def lookup(self, images_dev: DeviceArray, shape, lut: DeviceArray) -> DeviceArray:
        """nqk_image_lut of a uint8 device batch of `shape` (in this layout) through
        lut [C, 256]: the NCHW array of the table's dtype."""
        if self.layout == "NHWC":
            n, h, w, c = shape
        else:
            n, c, h, w = shape
        if images_dev.dtype != np.uint8 or images_dev.size != n * c * h * w:
            raise ValueError("image lookup: the device batch does not hold uint8 images of that shape")
        if tuple(lut.shape) != (c, 256):
            raise ValueError(f"image lookup: table of shape {lut.shape} for {c} channels")
        out = DeviceArray((n, c, h, w), lut.dtype)
        _lib.call("nqk_image_lut", images_dev.vp, lut.vp, lut.code, out.vp, n, h, w, c, _LAYOUTS[self.layout])
        return out

    def to_device(self, images: np.ndarray) -> FTensor:
        """`reference(images)` as an FTensor, computed on the device from the uint8 upload."""
        self.check(images)
        return FTensor(self.lookup(DeviceArray.from_host(images), images.shape, self.table_device()))


class QuantLut:
    """The quantized table of a QModel input: K.quantize(table, bit_width, scale, zp), kept
    until the preprocess values, the scale's bits, the zero point or the bit width change."""

    def __init__(self):
        self._key = None
        self._lut = None

    def get(self, pre: ImagePreprocess, bit_width: int, scale, zero_point) -> DeviceArray:
        zp = None if zero_point is None else int(zero_point)
        key = (pre.key(), np.float32(scale).tobytes(), zp, int(bit_width))
        if key != self._key:
            self._lut, _ = K.quantize(pre.table_device(), bit_width, scale, zp)
            self._key = key
        return self._lut


class PinnedBuffer:
    """Page-locked host memory (nqk_host_alloc) seen as a uint8 NumPy array."""

    def __init__(self, nbytes: int):
        _lib.ensure_init()
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        _lib.call("nqk_host_alloc", ctypes.byref(p), self.nbytes)
        self.ptr = p.value
        self.array = np.frombuffer((ctypes.c_uint8 * max(1, self.nbytes)).from_address(self.ptr), dtype=np.uint8)

    def free(self) -> None:
        if self.ptr:
            self.array = None
            _lib.call("nqk_host_free", ctypes.c_void_p(self.ptr))
            self.ptr = 0


def _event() -> ctypes.c_void_p:
    e = ctypes.c_void_p()
    _lib.call("nqk_event_create", ctypes.byref(e))
    return e


class UploadSlot:
    """One of classify_stream's two staging pairs: a pinned host buffer, a device buffer,
    the event the copy stream records after the upload (`copied`) and the event the library
    stream records after the kernel that read the device buffer (`read`)."""

    def __init__(self):
        self.host: PinnedBuffer | None = None
        self.dev: DeviceArray | None = None
        self.copied = _event()
        self.read = _event()
        self.read_pending = False
        self.shape = None

    def upload(self, images: np.ndarray) -> None:
        """Copy the batch into the pinned buffer and enqueue its upload on the copy stream,
        behind the kernel that last read this slot's device buffer.  Called on stream 0 with
        the side streams joined.  The caller has already received the results of the batch
        that last used this slot (a synchronous read-back behind its kernels), so that
        batch's upload from the pinned buffer has run."""
        nbytes = images.nbytes
        if self.host is None or self.host.nbytes < nbytes:
            if self.host is not None:
                self.host.free()
            self.host = PinnedBuffer(nbytes)
        if self.dev is None or self.dev.nbytes < nbytes:
            # The pool knows nothing of streams: the block it hands out may have been released
            # by a temporary whose kernel is still queued.  Stream order covers that for the
            # library's own streams, not for the copy stream, so the first upload into a new
            # block waits for everything issued so far.
            self.dev = DeviceArray((nbytes,), np.uint8)
            _lib.call("nqk_event_record", self.read)
            self.read_pending = True
        np.copyto(self.host.array[:nbytes].reshape(images.shape), images)
        if self.read_pending:
            _lib.call("nqk_upload_wait_for", self.read)
            self.read_pending = False
        _lib.call("nqk_upload_async", self.dev.vp, ctypes.c_void_p(self.host.ptr), nbytes, self.copied)
        self.shape = images.shape

    def images(self) -> DeviceArray:
        """The uploaded batch; the current stream waits for its copy."""
        _lib.call("nqk_event_wait", self.copied)
        return self.dev.offset_view(0, (int(np.prod(self.shape)),))

    def consumed(self) -> None:
        """After the kernel that reads `images()` was issued on the current stream."""
        _lib.call("nqk_event_record", self.read)
        self.read_pending = True

    def close(self) -> None:
        if self.host is not None:
            self.host.free()
            self.host = None
        self.dev = None
        for e in (self.copied, self.read):
            _lib.call("nqk_event_destroy", e)
