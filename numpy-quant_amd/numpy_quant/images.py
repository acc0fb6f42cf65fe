"""uint8 images as model inputs: per-channel normalize, layout change to NCHW and (for a
QModel) quantize, all as one table lookup on the device (nqk_image_lut).

`ImagePreprocess.reference` is the definition, in float32 NumPy.  Normalize and quantize
are elementwise per channel, so a uint8 pixel of channel c maps to one of 256 values:
`table()` holds the normalized ones, and `K.quantize(table, ...)` the quantized ones.  The
kernel gathers from the table and does no floating-point arithmetic, so its output is
`reference(img)` (or `quantize(reference(img))`) bit for bit.  The uint8 batch is a quarter
of the float32 one on the host link.

`ResizeCrop` puts Pillow's 8-bit bilinear resize and a center crop in front of that, for
batches of decoded photos of any sizes: an integer algorithm (`ResizeCrop.reference`, equal
to Pillow byte for byte) whose result is a uint8 again, so one kernel (nqk_image_resize_lut)
resizes, crops and looks up, and the bit-exactness above carries over.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import kernels as K
from .device import DeviceArray
from .tensor import FTensor

_LAYOUTS = {"NHWC": _lib.IMG_NHWC, "NCHW": _lib.IMG_NCHW}

PRECISION_BITS = 22  # Pillow's 8-bit resample: weights in 22-bit fixed point, int32 accumulator


def _pair(v, what: str) -> tuple[int, int]:
    if isinstance(v, (int, np.integer)):
        v = (v, v)
    if len(v) != 2 or not all(isinstance(s, (int, np.integer)) and s >= 1 for s in v):
        raise ValueError(f"ResizeCrop: {what} is a positive int or a pair of them, got {v!r}")
    return int(v[0]), int(v[1])


def _images_list(images) -> list:
    """A ragged batch as a list of 3-d arrays: a list / tuple as it is, a 4-d array by image."""
    if isinstance(images, np.ndarray):
        if images.ndim != 4:
            raise ValueError(f"ImagePreprocess: 4-d NHWC batch or a list of HWC images expected, got shape {images.shape}")
        return list(images)
    if isinstance(images, (list, tuple)):
        return list(images)
    raise ValueError(f"ImagePreprocess: a list of HWC uint8 images expected, got {type(images)}")


class ResizeCrop:
    """`ResizeCrop(size, crop=None)`: Pillow's 8-bit `Image.resize(..., BILINEAR)` followed by
    a center crop, byte for byte.  `size` as an int is the shorter side (the longer one is
    `int(size * long / short)`), as `(rh, rw)` the exact size; `crop` is an int or
    `(ch, cw)`, the center window of the resized image (`None`: all of it).

    The algorithm is integer: per axis, the taps of an output coordinate are computed in
    float64 and rounded to 22-bit fixed point (`taps`); the horizontal and then the vertical
    pass each accumulate in int32 from `1 << 21`, shift right by 22 and clip to 0..255.
    `reference` is that in NumPy; the device kernel (nqk_image_resize_lut) does the same
    arithmetic and finishes with the table lookup of ImagePreprocess.

    The kernel's caps, checked here before anything is uploaded: at most MAX_TAPS taps per
    axis (a downscale factor of 32), and the horizontally resized rows that one output row's
    vertical taps touch, `n_y * round_up(ow, 16) * c` bytes, within LDS_BYTES."""

    MAX_TAPS = 65          # NQK_RESIZE_MAX_TAPS
    LDS_BYTES = 56 << 10   # the kernel's budget for the intermediate rows of one tile

    def __init__(self, size, crop=None):
        self.size = int(size) if isinstance(size, (int, np.integer)) else _pair(size, "size")
        if isinstance(self.size, int) and self.size < 1:
            raise ValueError(f"ResizeCrop: size is a positive int or a pair of them, got {size!r}")
        self.crop = None if crop is None else _pair(crop, "crop")
        self._taps: dict[tuple, tuple[np.ndarray, np.ndarray]] = {}

    def __repr__(self):
        return f"ResizeCrop(size={self.size!r}, crop={self.crop!r})"

    # ------------------------------------------------------------------ sizes
    def resized(self, h: int, w: int) -> tuple[int, int]:
        """The size (rh, rw) an h x w image is resized to."""
        if h < 1 or w < 1:
            raise ValueError(f"ResizeCrop: empty image of {h} x {w}")
        if not isinstance(self.size, int):
            return self.size
        if h <= w:
            return self.size, int(self.size * w / h)
        return int(self.size * h / w), self.size

    def window(self, h: int, w: int) -> tuple[int, int, int, int, int, int]:
        """(rh, rw, top, left, oh, ow) of an h x w image: the resized size and the crop window."""
        rh, rw = self.resized(h, w)
        if rh < 1 or rw < 1:
            raise ValueError(f"ResizeCrop: a {h} x {w} image resizes to {rh} x {rw}")
        if self.crop is None:
            return rh, rw, 0, 0, rh, rw
        ch, cw = self.crop
        if ch > rh or cw > rw:
            raise ValueError(f"ResizeCrop: crop {ch} x {cw} is larger than the resized image {rh} x {rw} "
                             f"(from {h} x {w}); there is no padding")
        return rh, rw, int(round((rh - ch) / 2.0)), int(round((rw - cw) / 2.0)), ch, cw

    # ------------------------------------------------------------------ taps
    @staticmethod
    def tap_count(in_size: int, out_size: int) -> int:
        """ksize of the bilinear filter between these sizes"""
        return int(np.ceil(max(in_size / out_size, 1.0))) * 2 + 1

    def taps(self, in_size: int, out_size: int, first: int, count: int) -> tuple[np.ndarray, np.ndarray]:
        """Pillow's precompute_coeffs + normalize_coeffs_8bpc of the bilinear filter for the
        output coordinates first .. first + count of an axis resized from in_size to
        out_size: (bounds int32 [count, 2] = (first input index, tap count),
        weights int32 [count, ksize], zero past the tap count)."""
        key = (int(in_size), int(out_size), int(first), int(count))
        hit = self._taps.get(key)
        if hit is not None:
            return hit
        in_size, out_size, first, count = key
        if first < 0 or count < 1 or first + count > out_size:
            raise ValueError(f"ResizeCrop.taps: coordinates {first} .. {first + count} of {out_size}")
        scale = in_size / out_size
        filterscale = max(scale, 1.0)
        support = 1.0 * filterscale  # the bilinear filter's support is 1
        ksize = int(np.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
        xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
        n = xmax - xmin
        x = np.arange(ksize, dtype=np.int64)[None, :]
        w = 1.0 - np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
        w = np.where((w > 0.0) & (x < n[:, None]), w, 0.0)
        ww = np.zeros(count, dtype=np.float64)
        for k in range(ksize):  # the sum in Pillow's order
            ww = ww + w[:, k]
        w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
        fixed = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
        bounds = np.ascontiguousarray(np.stack([xmin, n], axis=1).astype(np.int32))
        hit = (bounds, np.ascontiguousarray(fixed))
        if len(self._taps) >= 256:
            self._taps.clear()
        self._taps[key] = hit
        return hit

    def check_cap(self, h: int, w: int, c: int) -> None:
        """ValueError if an h x w image of c channels is beyond what the kernel takes."""
        rh, rw, _, _, _, ow = self.window(h, w)
        kx, ky = self.tap_count(w, rw), self.tap_count(h, rh)
        if kx > self.MAX_TAPS or ky > self.MAX_TAPS:
            raise ValueError(f"ResizeCrop: {h} x {w} -> {rh} x {rw} needs {max(kx, ky)} taps, the kernel takes "
                             f"{self.MAX_TAPS} (a downscale factor of {(self.MAX_TAPS - 1) // 2})")
        rows = int(self.taps(h, rh, *self.window(h, w)[2::2])[0][:, 1].max())  # of one output row, at most
        need = rows * (-(-ow // 16) * 16) * c
        if need > self.LDS_BYTES:
            raise ValueError(f"ResizeCrop: {h} x {w} -> {rh} x {rw}: one output row of {ow} pixels needs "
                             f"{need} bytes of intermediate rows, the kernel holds {self.LDS_BYTES}")

    # ------------------------------------------------------------------ host definition
    def output_size(self, images) -> tuple[int, int]:
        """(oh, ow) of a batch; ValueError if its images give different ones."""
        sizes = {self.window(h, w)[4:] for h, w in {im.shape[:2] for im in images}}
        if len(sizes) != 1:
            raise ValueError(f"ResizeCrop: the images of one batch give different output sizes {sorted(sizes)}")
        return sizes.pop()

    @staticmethod
    def _resample(src: np.ndarray, bounds: np.ndarray, weights: np.ndarray) -> np.ndarray:
        """One pass along axis 0 of src [in, ...] uint8: [count, ...] uint8."""
        out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
        tail = (1,) * (src.ndim - 1)
        for i, (first, n) in enumerate(bounds):
            acc = (src[first:first + n].astype(np.int32) * weights[i, :n].reshape((n,) + tail)).sum(axis=0, dtype=np.int32)
            acc = (acc + np.int32(1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
            out[i] = np.clip(acc, 0, 255)
        return out

    def reference_one(self, image: np.ndarray) -> np.ndarray:
        """One HWC uint8 image resized and cropped: uint8 [oh, ow, c]."""
        h, w = image.shape[:2]
        rh, rw, top, left, oh, ow = self.window(h, w)
        xb, xw = self.taps(w, rw, left, ow)
        yb, yw = self.taps(h, rh, top, oh)
        mid = self._resample(image.transpose(1, 0, 2), xb, xw)  # [ow, h, c]
        return self._resample(mid.transpose(1, 0, 2), yb, yw)   # [oh, ow, c]

    def reference(self, images) -> np.ndarray:
        """The definition in integer NumPy: uint8 [n, oh, ow, c] of a list of HWC uint8
        images (or an NHWC batch): horizontal pass, vertical pass, crop."""
        images = _images_list(images)
        self.output_size(images)
        return np.ascontiguousarray(np.stack([self.reference_one(im) for im in images]))

    # ------------------------------------------------------------------ device batch
    def pack(self, images, c: int) -> "RaggedBatch":
        return RaggedBatch(self, images, c)


class RaggedBatch:
    """A list of HWC uint8 images laid out for nqk_image_resize_lut as one byte string:
    `meta` (n image descriptors of int64 offset, int32 h, w, xtab, ytab, then the int32 tap
    tables: ksize, count, bounds[count][2], weights[count][ksize] each; images of equal
    size share tables), padding to 16 bytes, then the pixels back to back."""

    def __init__(self, resize: ResizeCrop, images: list, c: int):
        self.n, self.c = len(images), c
        self.images = images
        self.oh, self.ow = resize.output_size(images)
        desc = np.zeros(self.n, dtype=np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("xtab", "<i4"),
                                                ("ytab", "<i4")]))
        tables, where, shapes, words, offset = [], {}, {}, 0, 0
        for i, im in enumerate(images):
            h, w = im.shape[:2]
            tab = shapes.get((h, w))
            if tab is None:
                rh, rw, top, left, oh, ow = resize.window(h, w)
                tab = []
                for key in ((w, rw, left, ow), (h, rh, top, oh)):
                    if key not in where:
                        bounds, weights = resize.taps(*key)
                        where[key] = words
                        tables += [np.array([weights.shape[1], key[3]], np.int32), bounds.reshape(-1), weights.reshape(-1)]
                        words += 2 + bounds.size + weights.size
                    tab.append(where[key])
                shapes[(h, w)] = tab
            desc[i] = (offset, h, w, tab[0], tab[1])
            offset += h * w * c
        self.meta = np.concatenate([desc.view(np.uint8)] + [t.view(np.uint8) for t in tables])
        self.pixel_offset = -(-self.meta.size // 16) * 16
        self.pixel_bytes = offset
        self.nbytes = self.pixel_offset + self.pixel_bytes

    def write(self, dst: np.ndarray) -> None:
        """The byte string into dst (uint8, nbytes long)."""
        dst[:self.meta.size] = self.meta
        pos = self.pixel_offset
        for im in self.images:
            np.copyto(dst[pos:pos + im.size].reshape(im.shape), im)
            pos += im.size


class ImagePreprocess:
    """`ImagePreprocess(mean, std, layout="NHWC", rescale=255, resize=None)`: per-channel (1
    to 4 channels) `((img / rescale) - mean) / std` of uint8 images given in `layout`.  With
    `resize` (a ResizeCrop) a batch is a list of HWC uint8 images of any sizes (or an NHWC
    array), each resized and center-cropped first, as Pillow would."""

    def __init__(self, mean, std, layout: str = "NHWC", rescale=255, resize: ResizeCrop | None = None):
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
        if resize is not None:
            if not isinstance(resize, ResizeCrop):
                raise ValueError(f"ImagePreprocess: resize is a ResizeCrop, got {type(resize)}")
            if layout != "NHWC":
                raise ValueError("ImagePreprocess: resize takes NHWC images")
        self.resize = resize
        self._table_dev = None
        self._stage = None  # host bytes of the last packed batch (resize_lookup_host)

    def __repr__(self):
        resize = "" if self.resize is None else f", resize={self.resize!r}"
        return (f"ImagePreprocess(mean={self.mean.tolist()}, std={self.std.tolist()}, layout={self.layout!r}, "
                f"rescale={float(self.rescale)}{resize})")

    @property
    def channels(self) -> int:
        return int(self.mean.size)

    def key(self) -> tuple:
        """The values a lookup table depends on (read on every call: the arrays are mutable)."""
        return (self.mean.tobytes(), self.std.tobytes(), self.rescale.tobytes())

    # ------------------------------------------------------------------ host definition
    def check(self, images) -> tuple[int, int, int, int]:
        """ValueError unless `images` is a non-empty 4-d uint8 batch of this channel count;
        returns (n, c, h, w).  With `resize`: a non-empty list or tuple of HWC uint8 images (or
        an NHWC batch), each within the kernel's caps and all of one output size; returns
        (n, c, oh, ow)."""
        if self.resize is not None:
            return self._check_ragged(_images_list(images))
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

    def _check_ragged(self, images: list) -> tuple[int, int, int, int]:
        if not images:
            raise ValueError("ImagePreprocess: empty batch")
        for im in images:
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8:
                raise ValueError(f"ImagePreprocess: uint8 images expected, got {getattr(im, 'dtype', type(im))}")
            if im.ndim != 3:
                raise ValueError(f"ImagePreprocess: 3-d HWC images expected, got shape {im.shape}")
            if im.shape[2] != self.channels:
                raise ValueError(f"ImagePreprocess: {im.shape[2]} channels in an image of shape {im.shape} (HWC), "
                                 f"{self.channels} in mean / std")
            if im.shape[0] == 0 or im.shape[1] == 0:
                raise ValueError(f"ImagePreprocess: empty image of shape {im.shape}")
        for h, w in {im.shape[:2] for im in images}:
            self.resize.check_cap(h, w, self.channels)
        oh, ow = self.resize.output_size(images)
        return len(images), self.channels, oh, ow

    def reference(self, images) -> np.ndarray:
        """The definition: float32 NCHW, float32 NumPy operations only (behind the integer
        `resize.reference` when a resize is set)."""
        self.check(images)
        if self.resize is not None:
            images = self.resize.reference(images)
        return self._normalize(images)

    def _normalize(self, images: np.ndarray) -> np.ndarray:
        bshape = (1, 1, 1, -1) if self.layout == "NHWC" else (1, -1, 1, 1)
        x = images.astype(np.float32) / self.rescale
        x = (x - self.mean.reshape(bshape)) / self.std.reshape(bshape)
        if self.layout == "NHWC":
            x = x.transpose(0, 3, 1, 2)
        return np.ascontiguousarray(x)

    def table(self) -> np.ndarray:
        """float32 [C, 256]: `reference` (without the resize, which maps uint8 to uint8 in
        front of it) of the values 0..255 in each channel."""
        v = np.arange(256, dtype=np.uint8)
        shape = (1, 1, 256, self.channels) if self.layout == "NHWC" else (1, self.channels, 1, 256)
        img = np.broadcast_to(v.reshape((1, 1, 256, 1) if self.layout == "NHWC" else (1, 1, 1, 256)), shape)
        return np.ascontiguousarray(self._normalize(np.ascontiguousarray(img)).reshape(self.channels, 256))

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

    def pack(self, images) -> RaggedBatch:
        """The checked batch of a preprocess with `resize`, laid out for the device."""
        if self.resize is None:
            raise ValueError("ImagePreprocess: no resize configured")
        images = _images_list(images)
        self._check_ragged(images)
        return self.resize.pack(images, self.channels)

    def lookup_resized(self, upload: DeviceArray, batch: RaggedBatch, meta_host, lut: DeviceArray) -> DeviceArray:
        """nqk_image_resize_lut of an uploaded RaggedBatch (`upload` holds batch.write's bytes,
        `meta_host` is the address of a host copy of them) through lut [C, 256]: the NCHW
        array [n, c, oh, ow] of the table's dtype."""
        if upload.dtype != np.uint8 or upload.size < batch.nbytes:
            raise ValueError("image resize: the device buffer does not hold the packed batch")
        if tuple(lut.shape) != (batch.c, 256):
            raise ValueError(f"image resize: table of shape {lut.shape} for {batch.c} channels")
        out = DeviceArray((batch.n, batch.c, batch.oh, batch.ow), lut.dtype)
        pixels = upload.offset_view(batch.pixel_offset, (batch.pixel_bytes,))
        _lib.call("nqk_image_resize_lut", pixels.vp, batch.pixel_bytes, upload.vp, ctypes.c_void_p(meta_host),
                  batch.meta.size, lut.vp, lut.code, out.vp, batch.n, batch.c, batch.oh, batch.ow)
        return out

    def resize_lookup_host(self, images, lut: DeviceArray) -> DeviceArray:
        """Pack, upload (synchronously) and look up a ragged batch."""
        batch = self.pack(images)
        if self._stage is None or self._stage.size < batch.nbytes:
            self._stage = np.empty(batch.nbytes, dtype=np.uint8)  # kept: fresh pages cost as much as the copy
        host = self._stage[:batch.nbytes]
        batch.write(host)
        return self.lookup_resized(DeviceArray.from_host(host), batch, host.ctypes.data, lut)

    def to_device(self, images) -> FTensor:
        """`reference(images)` as an FTensor, computed on the device from the uint8 upload."""
        if self.resize is not None:
            return FTensor(self.resize_lookup_host(images, self.table_device()))
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
        self.batch: RaggedBatch | None = None

    def upload(self, images) -> None:
        """Copy the batch into the pinned buffer and enqueue its upload on the copy stream,
        behind the kernel that last read this slot's device buffer.  Called on stream 0 with
        the side streams joined.  The caller has already received the results of the batch
        that last used this slot (a synchronous read-back behind its kernels), so that
        batch's upload from the pinned buffer has run."""
        ragged = isinstance(images, RaggedBatch)
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
        if ragged:  # descriptors, taps and pixels: one buffer, one copy
            images.write(self.host.array[:nbytes])
        else:
            np.copyto(self.host.array[:nbytes].reshape(images.shape), images)
        if self.read_pending:
            _lib.call("nqk_upload_wait_for", self.read)
            self.read_pending = False
        _lib.call("nqk_upload_async", self.dev.vp, ctypes.c_void_p(self.host.ptr), nbytes, self.copied)
        self.batch, self.shape = (images, (nbytes,)) if ragged else (None, images.shape)

    def images(self) -> DeviceArray:
        """The uploaded batch (a RaggedBatch: its whole byte string; `batch` is the layout and
        `host.ptr` the host copy of its descriptors); the current stream waits for its copy."""
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
