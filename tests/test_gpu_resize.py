"""GPU: ragged uint8 images resized, center-cropped and looked up on the device
(nqk_image_resize_lut) against `ResizeCrop.reference` + a NumPy gather, bit for bit; the
entry point's host-side validation; and a ViT at batch 2 fed lists of images through
QModel, Model and classify_stream against the float32 path."""
import ctypes

import numpy as np
import pytest

from test_gpu_images import (IMAGENET, SENTINEL, SLACK, _current_stream, _gather, _input_equals_quantize_tensor, _lut,
                             _raw, _stream0)

pytestmark = pytest.mark.gpu

DESC = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("xtab", "<i4"), ("ytab", "<i4")])


def _ragged(shapes, c, seed=0):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, size=tuple(s) + (c,), dtype=np.uint8) for s in shapes]
    imgs[0].reshape(-1)[:3] = (0, 255, 255)  # the ends of the range are there
    return imgs


def _upload(batch, px_shift=0):
    """The packed batch as (host bytes, pixel offset), the pixels moved px_shift bytes on"""
    host = np.zeros(batch.nbytes + px_shift, np.uint8)
    batch.write(host[:batch.nbytes])
    if px_shift:
        host[batch.pixel_offset + px_shift:] = host[batch.pixel_offset:batch.nbytes].copy()
        host[batch.pixel_offset:batch.pixel_offset + px_shift] = 0xEE
    return host, batch.pixel_offset + px_shift


def _call(batch, dev, px_off, host_bytes, lut_dev, out_dev, **over):
    from numpy_quant import _lib
    args = dict(pixels=dev.offset_view(px_off, (batch.pixel_bytes,)).vp, pixel_bytes=batch.pixel_bytes, meta_dev=dev.vp,
                meta_host=ctypes.c_void_p(host_bytes.ctypes.data), meta_bytes=batch.meta.size, lut=lut_dev.vp,
                lut_dtype=lut_dev.code, out=out_dev.vp, n=batch.n, c=batch.c, oh=batch.oh, ow=batch.ow)
    args.update(over)
    _lib.call("nqk_image_resize_lut", *args.values())


def _run_resize(imgs, rc, lut, px_shift=0, out_shift=0):
    """nqk_image_resize_lut of the packed images, the output an offset view (out_shift elements
    past the slack) into a sentinel-filled buffer; returns (out NCHW, want)."""
    from numpy_quant.device import DeviceArray
    c = lut.shape[0]
    batch = rc.pack(imgs, c)
    host, px_off = _upload(batch, px_shift)
    dev = DeviceArray.from_host(host)
    total = batch.n * c * batch.oh * batch.ow
    buf_host = np.full(SLACK + out_shift + total + SLACK, SENTINEL, dtype=lut.dtype)
    buf = DeviceArray.from_host(buf_host)
    lut_dev = DeviceArray.from_host(lut)
    lo, hi = SLACK + out_shift, SLACK + out_shift + total
    _call(batch, dev, px_off, host, lut_dev, buf.offset_view(lo, (batch.n, c, batch.oh, batch.ow)))
    got = buf.to_host()
    np.testing.assert_array_equal(_raw(got[:lo]), _raw(buf_host[:lo]), err_msg="write in front of the output")
    np.testing.assert_array_equal(_raw(got[hi:]), _raw(buf_host[hi:]), err_msg="write behind the output")
    want = _gather(lut, rc.reference(imgs).transpose(0, 3, 1, 2))
    assert want.shape == (batch.n, c, batch.oh, batch.ow)
    return got[lo:hi].reshape(want.shape), want


# id: (source sizes (h, w), size, crop, channels, table dtype, pixel shift, output shift)
KERNEL_CASES = {
    "1x1":             ([(5, 7)], (1, 1), None, 3, np.int8, 0, 0),
    "ow15":            ([(9, 20), (9, 21)], (4, 15), None, 3, np.int8, 1, 0),
    # oh = 17 crosses the 16-row tile; planes of 17 * 16 bytes keep every row's store aligned
    "ow16-oh17":       ([(20, 33), (31, 16), (23, 40)], (17, 16), None, 3, np.int8, 0, 0),
    "ow16-oh17-shift": ([(20, 33), (31, 16)], (17, 16), None, 3, np.int8, 1, 3),  # unaligned output base
    "ow17":            ([(12, 30), (7, 19)], (5, 17), None, 3, np.int8, 0, 0),    # every second row unaligned
    "ow48":            ([(30, 100), (25, 97)], (17, 48), None, 3, np.int8, 1, 0),
    "ow48-1ch":        ([(30, 100), (25, 97)], (17, 48), None, 1, np.int8, 0, 16),
    "ow48-4ch":        ([(30, 100), (25, 97)], (17, 48), None, 4, np.int8, 3, 0),
    "src-h1":          ([(1, 9), (1, 1)], (4, 6), None, 3, np.int8, 0, 0),
    "src-w1":          ([(9, 1), (2, 1)], (6, 4), None, 3, np.int8, 1, 0),
    # 105, 27, 105 bytes: odd offsets between the images
    "odd-offsets":     ([(5, 7), (3, 3), (7, 5), (2, 2)], (8, 8), None, 3, np.int8, 0, 0),
    "identity":        ([(33, 47)], (33, 47), None, 3, np.int8, 0, 0),
    "upscale3":        ([(11, 13)], (33, 39), None, 3, np.int8, 0, 0),
    # factor 16 both ways: 16 output rows would touch 288 rows of 48 * 3 bytes, the tile shrinks to 8
    "down16-tall":     ([(272, 768)], (17, 48), None, 3, np.int8, 1, 0),
    # two output rows touch 32 rows of 304 * 4 bytes, one 24: the tile shrinks to one row
    "down16-wide-4ch": ([(32, 608)], (2, 304), None, 4, np.int8, 0, 0),
    # one output row's 48 rows of 304 * 3 bytes: past the budget aimed at, within the cap
    "down32-hard":     ([(64, 608)], (2, 304), None, 3, np.int8, 0, 0),
    "shorter-side":    ([(30, 40), (26, 25), (50, 25)], 25, 22, 3, np.int8, 0, 0),
    "crop-odd-left":   ([(10, 19), (20, 38)], 20, 16, 3, np.int8, 0, 0),           # 20 x 38: top 2, left 11
    "crop-odd-left-w": ([(10, 19)], 20, (3, 17), 3, np.int16, 0, 0),              # left round(10.5) = 10, top 8
    "int16":           ([(9, 20), (12, 11)], (5, 17), None, 3, np.int16, 1, 1),
    "int32":           ([(9, 20), (12, 11)], (5, 17), None, 3, np.int32, 0, 0),
    "int64":           ([(9, 20), (12, 11)], (5, 17), None, 3, np.int64, 1, 0),
    "float32":         ([(9, 20), (12, 11)], (18, 17), None, 3, np.float32, 0, 1),
    "float32-1ch":     ([(9, 20), (12, 11)], (5, 16), None, 1, np.float32, 0, 0),
    "int64-4ch":       ([(9, 20), (12, 11)], (5, 15), None, 4, np.int64, 0, 0),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES), ids=list(KERNEL_CASES))
def test_resize_lut_kernel(case):
    from numpy_quant.images import ResizeCrop
    shapes, size, crop, c, dtype, px_shift, out_shift = KERNEL_CASES[case]
    rc = ResizeCrop(size, crop)
    if case.startswith("crop-odd-left"):
        assert rc.window(*shapes[0])[3] % 2 == (1 if case == "crop-odd-left" else 0) and rc.window(*shapes[0])[2] > 0
    got, want = _run_resize(_ragged(shapes, c, seed=len(case)), rc, _lut(c, dtype, seed=c), px_shift, out_shift)
    assert not np.any(_raw(want) == _raw(np.array(SENTINEL, dtype=want.dtype)))
    np.testing.assert_array_equal(_raw(got), _raw(want))


def test_resize_lut_invalid_arguments():
    """Every condition the entry point checks on the host, with a wrong table in the host copy
    only (the device copy stays the valid one): an error, and nothing written."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.images import ResizeCrop
    rc = ResizeCrop((6, 10), None)
    imgs = _ragged([(12, 17), (9, 30)], 3, seed=7)
    lut = _lut(3, np.int8, seed=7)
    batch = rc.pack(imgs, 3)
    host, px_off = _upload(batch)
    dev = DeviceArray.from_host(host)
    lut_dev = DeviceArray.from_host(lut)
    total = batch.n * 3 * 6 * 10
    buf_host = np.full(SLACK + total + SLACK, SENTINEL, np.int8)
    buf = DeviceArray.from_host(buf_host)
    out = buf.offset_view(SLACK, (batch.n, 3, 6, 10))

    nd = batch.n * DESC.itemsize
    words = (batch.meta.size - nd) // 4

    def wrong(edit):
        """a copy of the host bytes with edit(descriptors, taps) applied"""
        bad = host.copy()
        edit(bad[:nd].view(DESC), bad[nd:batch.meta.size].view(np.int32))
        return bad

    def field(i, name, value):
        def edit(desc, taps):
            desc[name][i] = value
        return edit

    def tap(image, axis, where, value):
        """word `where` of the image's x / y table: 0 ksize, 1 count, 2 + 2 i first, 3 + 2 i n;
        negative: from the table's end (the weights)"""
        def edit(desc, taps):
            t = int(desc[axis][image])
            size = 2 + 2 * int(taps[t + 1]) + int(taps[t + 1]) * int(taps[t])
            taps[t + (where if where >= 0 else size + where)] = value
        return edit

    ytab1 = int(host[:nd].view(DESC)["ytab"][1])
    ksize_y1 = int(host[nd:batch.meta.size].view(np.int32)[ytab1])
    assert ksize_y1 == 5 and words > 0
    edits = {
        "offset past the buffer": field(1, "offset", batch.pixel_bytes - 9 * 30 * 3 + 1),
        "offset negative": field(0, "offset", -1),
        "h too large": field(1, "h", 10),
        "w too large": field(1, "w", 31),
        "h zero": field(0, "h", 0),
        "w negative": field(0, "w", -3),
        "xtab negative": field(0, "xtab", -1),
        "xtab past the blob": field(0, "xtab", words - 1),
        "ytab past the blob": field(1, "ytab", words),
        "ytab extends past the blob": field(1, "ytab", words - 4),
        "xtab is the y table": field(0, "xtab", int(host[:nd].view(DESC)["ytab"][0])),  # count 6, not 10
        "ksize zero": tap(0, "xtab", 0, 0),
        "ksize above the cap": tap(0, "xtab", 0, 66),
        "ksize larger than the blob holds": tap(1, "ytab", 0, 40),
        "count wrong": tap(0, "ytab", 1, 5),
        "first negative": tap(0, "xtab", 2, -1),
        "first + n past w": tap(0, "xtab", 2 + 2 * 9, 16),
        "first + n past h": tap(1, "ytab", 2 + 2 * 5, 8),
        "n above ksize": tap(1, "ytab", 3 + 2 * 2, ksize_y1 + 1),
        "n negative": tap(1, "ytab", 3, -1),
        "weights overflow the accumulator": tap(0, "xtab", 2 + 2 * 10, (1 << 23) + (1 << 20)),
        "negative weights overflow it too": tap(0, "xtab", 2 + 2 * 10, -(1 << 24)),
    }
    _call(batch, dev, px_off, host, lut_dev, out)  # the valid call
    want = _gather(lut, rc.reference(imgs).transpose(0, 3, 1, 2))
    np.testing.assert_array_equal(buf.to_host()[SLACK:SLACK + total].reshape(want.shape), want)
    _lib.call("nqk_memset", buf.vp, SENTINEL, buf.nbytes)
    for what, edit in edits.items():
        with pytest.raises(_lib.NQKError):
            _call(batch, dev, px_off, wrong(edit), lut_dev, out)
            pytest.fail(f"accepted: {what}")
    odd = np.zeros(host.size + 8, np.uint8)
    odd[4:4 + host.size] = host
    for what, over in {
        "c = 0": dict(c=0), "c = 5": dict(c=5), "c does not match the buffer": dict(c=4),
        "n = 0": dict(n=0), "n larger than the descriptors": dict(n=batch.n + 1000),
        "oh is not the table's count": dict(oh=7), "ow is not the table's count": dict(ow=9), "ow = 0": dict(ow=0),
        "pixel buffer smaller": dict(pixel_bytes=batch.pixel_bytes - 1), "pixel buffer empty": dict(pixel_bytes=0),
        "meta too short": dict(meta_bytes=nd - 8), "meta no whole words": dict(meta_bytes=batch.meta.size - 2),
        "meta cut": dict(meta_bytes=batch.meta.size - 4),
        "meta host misaligned": dict(meta_host=ctypes.c_void_p(odd.ctypes.data + 4)),
        "meta device misaligned": dict(meta_dev=dev.offset_view(4, (8,)).vp),
        "null pixels": dict(pixels=None), "null meta": dict(meta_dev=None), "null host meta": dict(meta_host=None),
        "null table": dict(lut=None), "null output": dict(out=None),
        "dtype 0": dict(lut_dtype=0), "dtype 6": dict(lut_dtype=6),
    }.items():
        with pytest.raises(_lib.NQKError):
            _call(batch, dev, px_off, host, lut_dev, out, **over)
            pytest.fail(f"accepted: {what}")
    np.testing.assert_array_equal(buf.to_host(), buf_host, err_msg="a refused call wrote something")
    _call(batch, dev, px_off, host, lut_dev, out)  # and the valid one still runs
    np.testing.assert_array_equal(buf.to_host()[SLACK:SLACK + total].reshape(want.shape), want)


def test_resize_lut_refuses_rows_beyond_the_lds_cap():
    """A table the Python side would refuse (ResizeCrop.check_cap), given to the entry point:
    32 rows of 2800 * 4 bytes for one output row."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray
    from numpy_quant.images import ResizeCrop
    rc = ResizeCrop((1, 2800))
    img = np.zeros((32, 2800, 4), np.uint8)
    with pytest.raises(ValueError, match="intermediate"):
        rc.check_cap(32, 2800, 4)
    batch = rc.pack([img], 4)
    host, px_off = _upload(batch)
    dev = DeviceArray.from_host(host)
    out = DeviceArray((1, 4, 1, 2800), np.int8)
    with pytest.raises(_lib.NQKError, match="NQK_RESIZE_LDS_BYTES"):
        _call(batch, dev, px_off, host, DeviceArray.from_host(_lut(4, np.int8)), out)


def test_to_device_is_reference():
    from numpy_quant.images import ImagePreprocess, ResizeCrop
    from numpy_quant.tensor import FTensor
    pre = ImagePreprocess(*IMAGENET, resize=ResizeCrop(25, 22))
    imgs = _ragged([(30, 40), (26, 25), (61, 25)], 3, seed=3)
    for batch in (imgs, tuple(imgs), np.stack([imgs[0], imgs[0][::-1]])):
        t = pre.to_device(batch)
        assert isinstance(t, FTensor)
        np.testing.assert_array_equal(_raw(t.data), _raw(pre.reference(batch)))
    pre.mean[0] = 0.25  # the device table follows the values
    np.testing.assert_array_equal(_raw(pre.to_device(imgs).data), _raw(pre.reference(imgs)))
    with pytest.raises(ValueError):
        pre.to_device([imgs[0].astype(np.float32)])
    with pytest.raises(ValueError, match="different output sizes"):
        ImagePreprocess(*IMAGENET, resize=ResizeCrop(25)).to_device(imgs)


# ----------------------------------------------------------------------------- ViT, batch 2
@pytest.fixture(scope="module")
def vit():
    from numpy_quant.images import ImagePreprocess, ResizeCrop
    from test_gpu_plan import _vit
    pre = ImagePreprocess(*IMAGENET, resize=ResizeCrop(256, 224))
    batches = [_ragged([(300, 400), (260, 256)], 3, seed=20 + k) for k in range(3)]
    refs = [pre.reference(b) for b in batches]  # computed once, left unchanged
    for r in refs:
        assert r.shape == (2, 3, 224, 224)
        r.setflags(write=False)
    return _vit(2), pre, batches, refs


@pytest.fixture(scope="module")
def vit_q8(vit):
    model, pre, batches, refs = vit
    return model.quantize([refs[0]], bit_width=8)


@pytest.mark.parametrize("bw", [8, 4])
def test_vit_image_list_equals_float_path(vit, vit_q8, bw):
    model, pre, batches, refs = vit
    qmodel = vit_q8 if bw == 8 else model.quantize([refs[0]], bit_width=4)
    plain = type(pre)(*IMAGENET)
    for without in (None, plain):  # a list needs a resize: ValueError, not AttributeError
        qmodel.image_preprocess = without
        with pytest.raises(ValueError, match="resize"):
            qmodel([batches[0]])
    qmodel.image_preprocess = pre
    plan = qmodel.compile()
    assert plan.fused == 12
    want = qmodel([refs[0]])[0]
    np.testing.assert_array_equal(_raw(qmodel([batches[0]])[0]), _raw(want))
    _input_equals_quantize_tensor(qmodel, refs[0])
    np.testing.assert_array_equal(_raw(qmodel([tuple(batches[0])])[0]), _raw(want))
    qmodel.keep_values = True
    try:
        eager_want = qmodel([refs[0]])[0]
        np.testing.assert_array_equal(_raw(qmodel([batches[0]])[0]), _raw(eager_want))
        _input_equals_quantize_tensor(qmodel, refs[0])
    finally:
        qmodel.keep_values = False


def test_vit_float_model_and_calibration_from_lists(vit, vit_q8):
    model, pre, batches, refs = vit
    with pytest.raises(ValueError, match="resize"):
        model([batches[0]])
    model.image_preprocess = pre
    try:
        np.testing.assert_array_equal(_raw(pre.to_device(batches[0]).data), _raw(refs[0]))
        q = model.quantize([batches[0]], bit_width=8)
        np.testing.assert_array_equal(_raw(model.inputs[0].data.data), _raw(refs[0]))
    finally:
        model.image_preprocess = None
    assert q.image_preprocess is pre
    assert set(q.quant_params) == set(vit_q8.quant_params)
    for name, want in vit_q8.quant_params.items():
        got = q.quant_params[name]
        assert np.float32(got.scale).tobytes() == np.float32(want.scale).tobytes(), name
        assert (got.zero_point is None) == (want.zero_point is None), name
        if want.zero_point is not None:
            assert int(got.zero_point) == int(want.zero_point), name


def test_classify_stream_ragged(vit, vit_q8):
    model, pre, batches, refs = vit
    qmodel = vit_q8
    qmodel.image_preprocess = pre
    want = [qmodel([b])[0] for b in batches]
    for w, r in zip(want, refs):
        np.testing.assert_array_equal(_raw(w), _raw(qmodel([r])[0]))
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    s0 = _stream0()
    got = list(qmodel.classify_stream(iter(batches)))
    assert len(got) == 3
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_raw(g), _raw(w))
    assert _current_stream() == s0
    # a batch the preprocess refuses, mid-stream: after the result of the batch before it, and
    # the library is back on stream 0
    stream = qmodel.classify_stream([batches[1], [batches[0][0], batches[0][1][..., :2]], batches[2]])
    np.testing.assert_array_equal(_raw(next(stream)), _raw(want[1]))
    with pytest.raises(ValueError, match="channels"):
        next(stream)
    with pytest.raises(StopIteration):
        next(stream)
    assert _current_stream() == s0
    np.testing.assert_array_equal(_raw(qmodel([batches[2]])[0]), _raw(want[2]))
