"""CPU: the host definition of resize + center crop (numpy_quant/images.py ResizeCrop).
`reference` is Pillow's 8-bit bilinear resize restated in integer NumPy: compared byte for
byte with bytes Pillow wrote (tests/golden/resize_pillow.npz, make_resize_golden.py), and
with the installed Pillow where there is one."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from numpy_quant.images import ImagePreprocess, RaggedBatch, ResizeCrop

IMAGENET = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
FIX = np.load(os.path.join(GOLDEN, "resize_pillow.npz"))
CASES = [tuple(int(v) for v in row) for row in FIX["cases"]]  # (h, w, oh, ow, c)
CASE_IDS = [f"{h}x{w}x{c}-{oh}x{ow}" for h, w, oh, ow, c in CASES]

# (image h, w), size, crop -> (rh, rw, top, left, oh, ow), computed by hand:
# int(256 * 500 / 375) = int(341.33) = 341; round(117 / 2) = round(58.5) = 58 (half to even)
WINDOWS = [
    ((375, 500), 256, 224, (256, 341, 16, 58, 224, 224)),
    ((500, 375), 256, 224, (341, 256, 58, 16, 224, 224)),
    ((300, 400), 256, 224, (256, 341, 16, 58, 224, 224)),
    ((260, 256), 256, 224, (260, 256, 18, 16, 224, 224)),   # w < h: int(256 * 260 / 256) = 260
    ((333, 500), 256, 224, (256, 384, 16, 80, 224, 224)),   # int(384.38)
    ((480, 640), (224, 224), None, (224, 224, 0, 0, 224, 224)),
    ((100, 100), 256, (224, 200), (256, 256, 16, 28, 224, 200)),
    ((37, 53), 64, 63, (64, 91, 0, 14, 63, 63)),            # int(91.68); round(0.5) = 0
    ((37, 53), 64, 61, (64, 91, 2, 15, 61, 61)),            # round(1.5) = 2
    ((5, 5), 8, None, (8, 8, 0, 0, 8, 8)),
]
AXES = sorted({(h, oh) for h, w, oh, ow, c in CASES} | {(w, ow) for h, w, oh, ow, c in CASES}
              | {(hw[0], win[0]) for hw, _, _, win in WINDOWS} | {(hw[1], win[1]) for hw, _, _, win in WINDOWS}
              | {(1000, 256), (1333, 341), (3, 224), (600, 75), (2080, 65), (1, 1)})


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_reference_is_pillow_recorded(i):
    h, w, oh, ow, c = CASES[i]
    img, want = FIX[f"in{i}"], FIX[f"out{i}"]
    assert img.shape == (h, w, c) and want.shape == (oh, ow, c)
    got = ResizeCrop((oh, ow)).reference([img])
    assert got.dtype == np.uint8 and got.shape == (1, oh, ow, c) and got.flags.c_contiguous
    np.testing.assert_array_equal(got[0], want)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_reference_is_pillow_installed(i):
    Image = pytest.importorskip("PIL.Image")
    h, w, oh, ow, c = CASES[i]
    img = FIX[f"in{i}"]
    pil = Image.fromarray(img[..., 0] if c == 1 else img)
    want = np.asarray(pil.resize((ow, oh), Image.BILINEAR)).reshape(oh, ow, c)
    np.testing.assert_array_equal(want, FIX[f"out{i}"], err_msg="the installed Pillow differs from the recorded one")
    np.testing.assert_array_equal(ResizeCrop((oh, ow)).reference([img])[0], want)


def test_fixture_covers_what_it_should():
    assert os.path.getsize(os.path.join(GOLDEN, "resize_pillow.npz")) < 100_000
    assert str(FIX["pillow_version"])
    assert {c for *_, c in CASES} == {1, 3}
    taps = {max(ResizeCrop.tap_count(h, oh), ResizeCrop.tap_count(w, ow)) for h, w, oh, ow, c in CASES}
    assert min(taps) == 3 and max(taps) == 33  # upscale / identity ... factor 16


@pytest.mark.parametrize("hw,size,crop,want", WINDOWS, ids=[f"{a[0]}x{a[1]}-{s}-{c}" for a, s, c, _ in WINDOWS])
def test_window_arithmetic(hw, size, crop, want):
    rc = ResizeCrop(size, crop)
    assert rc.window(*hw) == want
    assert rc.resized(*hw) == want[:2]
    img = np.zeros(hw + (3,), np.uint8)
    assert rc.output_size([img]) == want[4:]
    assert ImagePreprocess(*IMAGENET, resize=rc).check([img, img]) == (2, 3) + want[4:]


def test_crop_is_a_window_of_the_resized_image():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    full = ResizeCrop(64).reference([img])[0]
    assert full.shape == (64, 91, 3)
    for crop, top, left in ((63, 0, 14), (61, 2, 15), ((10, 91), 27, 0), ((64, 1), 0, 45)):
        rc = ResizeCrop(64, crop)
        got = rc.reference([img])[0]
        ch, cw = (crop, crop) if isinstance(crop, int) else crop
        assert rc.window(37, 53)[2:] == (top, left, ch, cw)
        np.testing.assert_array_equal(got, full[top:top + ch, left:left + cw])


@pytest.mark.parametrize("in_size,out_size", AXES, ids=lambda v: str(v))
def test_taps_within_bounds(in_size, out_size):
    """what nqk_image_resize_lut checks of a table, and the written formula for one coordinate"""
    rc = ResizeCrop(1)
    bounds, weights = rc.taps(in_size, out_size, 0, out_size)
    ksize = ResizeCrop.tap_count(in_size, out_size)
    assert bounds.dtype == np.int32 and weights.dtype == np.int32
    assert bounds.shape == (out_size, 2) and weights.shape == (out_size, ksize)
    first, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert np.all(first >= 0) and np.all(n >= 1) and np.all(n <= ksize) and np.all(first + n <= in_size)
    assert np.all(255 * np.abs(weights.astype(np.int64)).sum(axis=1) + (1 << 21) < (1 << 31))
    assert np.all(weights[np.arange(ksize)[None, :] >= n[:, None]] == 0)
    assert np.all(np.abs(weights.astype(np.int64).sum(axis=1) - (1 << 22)) <= ksize)
    # a part of the axis is the same rows (the crop window's tables)
    lo, cnt = out_size // 3, max(1, out_size // 2)
    b2, w2 = rc.taps(in_size, out_size, lo, cnt)
    np.testing.assert_array_equal(b2, bounds[lo:lo + cnt])
    np.testing.assert_array_equal(w2, weights[lo:lo + cnt])
    assert rc.taps(in_size, out_size, lo, cnt)[0] is b2  # cached
    # the last coordinate, in scalar Python floats
    xx = out_size - 1
    scale = in_size / out_size
    fs = max(scale, 1.0)
    center = (xx + 0.5) * scale
    xmin = max(int(center - fs + 0.5), 0)
    xmax = min(int(center + fs + 0.5), in_size)
    k = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * (1.0 / fs))) for x in range(xmax - xmin)]
    ww = 0.0
    for v in k:
        ww += v
    assert (first[xx], n[xx]) == (xmin, xmax - xmin)
    assert weights[xx, :xmax - xmin].tolist() == [int(0.5 + v / ww * (1 << 22)) for v in k]


def test_identity_taps_reproduce_the_byte():
    bounds, weights = ResizeCrop(1).taps(47, 47, 0, 47)
    assert weights.shape == (47, 3)
    assert np.all(bounds[:, 1] <= 2)
    for i in range(47):
        assert weights[i].tolist().count(1 << 22) == 1 and weights[i].sum() == 1 << 22


def test_ragged_batch_layout():
    rng = np.random.default_rng(1)
    shapes = [(5, 7), (9, 3), (5, 7), (11, 11)]
    imgs = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
    imgs[1] = np.asfortranarray(imgs[1])  # not contiguous: packed all the same
    rc = ResizeCrop((6, 6), 4)
    batch = ImagePreprocess(*IMAGENET, resize=rc).pack(imgs)
    assert isinstance(batch, RaggedBatch) and (batch.n, batch.c, batch.oh, batch.ow) == (4, 3, 4, 4)
    buf = np.full(batch.nbytes + 8, 0xEE, np.uint8)
    batch.write(buf[:batch.nbytes])
    assert np.all(buf[batch.nbytes:] == 0xEE)
    assert batch.pixel_offset % 16 == 0 and batch.pixel_offset >= batch.meta.size
    assert batch.pixel_bytes == sum(im.size for im in imgs)
    desc = buf[:4 * 24].view(np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("xtab", "<i4"), ("ytab", "<i4")]))
    taps = buf[4 * 24:batch.meta.size].view(np.int32)
    assert desc["offset"].tolist() == [0, 105, 186, 291]  # odd byte offsets
    assert desc[0]["xtab"] == desc[2]["xtab"] and desc[0]["ytab"] == desc[2]["ytab"]  # shared
    assert len({int(d[k]) for d in desc for k in ("xtab", "ytab")}) == 5  # 7, 5, 3, 9 and 11 -> 6 (11 x 11 shares one)
    for d, im in zip(desc, imgs):
        assert (d["h"], d["w"]) == im.shape[:2]
        px = buf[batch.pixel_offset + d["offset"]:][:im.size].reshape(im.shape)
        np.testing.assert_array_equal(px, im)
        for tab, in_size in ((d["xtab"], im.shape[1]), (d["ytab"], im.shape[0])):
            ksize, count = taps[tab], taps[tab + 1]
            bounds, weights = rc.taps(in_size, 6, 1, 4)
            assert (ksize, count) == (weights.shape[1], 4)
            np.testing.assert_array_equal(taps[tab + 2:tab + 10].reshape(4, 2), bounds)
            np.testing.assert_array_equal(taps[tab + 10:tab + 10 + 4 * ksize].reshape(4, ksize), weights)


def test_preprocess_reference_and_repr():
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((30, 40), (26, 25))]
    rc = ResizeCrop(25, 22)
    pre = ImagePreprocess(*IMAGENET, resize=rc)
    plain = ImagePreprocess(*IMAGENET)
    assert pre.check(imgs) == (2, 3, 22, 22) and pre.check(tuple(imgs)) == (2, 3, 22, 22)
    u8 = rc.reference(imgs)
    assert u8.shape == (2, 22, 22, 3)
    np.testing.assert_array_equal(pre.reference(imgs).view(np.uint32), plain.reference(u8).view(np.uint32))
    batch = np.stack([imgs[0], imgs[0][::-1]])  # a 4-d NHWC batch is a list of its images
    np.testing.assert_array_equal(rc.reference(batch), rc.reference(list(batch)))
    assert pre.check(batch) == (2, 3, 22, 22)
    assert pre.key() == plain.key()
    np.testing.assert_array_equal(pre.table().view(np.uint32), plain.table().view(np.uint32))
    assert "resize" not in repr(plain)
    assert repr(pre).endswith("resize=ResizeCrop(size=25, crop=(22, 22)))")


def test_validation_errors():
    img = np.zeros((30, 40, 3), np.uint8)
    pre = ImagePreprocess(*IMAGENET, resize=ResizeCrop(25, 22))
    assert pre.check([img]) == (1, 3, 22, 22)
    bad_batches = [
        [],                                              # an empty batch
        [np.zeros((30, 0, 3), np.uint8)],                # an empty image
        [np.zeros((0, 40, 3), np.uint8)],
        [img, np.zeros((30, 40, 4), np.uint8)],          # wrong channel count
        [img[..., 0]],                                   # not HWC
        [img.astype(np.float32)],
        [[1, 2, 3]],
        img,                                             # a single 3-d array is no batch
        "images",
    ]
    for bad in bad_batches:
        with pytest.raises(ValueError):
            pre.check(bad)
        with pytest.raises(ValueError):
            pre.reference(bad)
        with pytest.raises(ValueError):
            pre.pack(bad)
    # a crop larger than the resized image: 20 x 26 from 30 x 40
    with pytest.raises(ValueError, match="larger than the resized image"):
        ImagePreprocess(*IMAGENET, resize=ResizeCrop(20, 22)).check([img])
    with pytest.raises(ValueError, match="larger than the resized image"):
        ResizeCrop(20, 22).reference([img])
    # mixed output sizes in one batch (no crop: 25 x 33 and 25 x 25)
    loose = ImagePreprocess(*IMAGENET, resize=ResizeCrop(25))
    with pytest.raises(ValueError, match="different output sizes"):
        loose.check([img, np.zeros((30, 30, 3), np.uint8)])
    with pytest.raises(ValueError, match="different output sizes"):
        loose.resize.reference([img, np.zeros((30, 30, 3), np.uint8)])
    # NCHW with resize
    with pytest.raises(ValueError, match="NHWC"):
        ImagePreprocess(*IMAGENET, layout="NCHW", resize=ResizeCrop(25, 22))
    with pytest.raises(ValueError):
        ImagePreprocess(*IMAGENET, resize=(25, 22))
    for size, crop in ((0, None), ((4, 0), None), (8, 0), ((1, 2, 3), None), (8, (1, 2, 3))):
        with pytest.raises(ValueError):
            ResizeCrop(size, crop)


def test_scale_cap():
    """MAX_TAPS taps per axis (a downscale factor of 32), and one output row's intermediate
    rows within LDS_BYTES"""
    assert ResizeCrop.MAX_TAPS == 65 and ResizeCrop.LDS_BYTES == 56 << 10
    one = ImagePreprocess([0.5], [0.5], resize=ResizeCrop((2, 2)))
    assert one.check([np.zeros((64, 32, 1), np.uint8)]) == (1, 1, 2, 2)        # factor 32 and 16
    for shape in ((66, 4, 1), (4, 66, 1)):                                       # factor 33: 67 taps
        with pytest.raises(ValueError, match="taps"):
            one.check([np.zeros(shape, np.uint8)])
        with pytest.raises(ValueError, match="taps"):
            one.resize.check_cap(shape[0], shape[1], 1)
    ResizeCrop(256, 224).check_cap(4096, 4096, 4)                               # factor 16, 4 channels
    ResizeCrop((3, 4)).check_cap(48, 64, 3)
    ResizeCrop((900, 900)).check_cap(3, 3, 4)                                   # any upscale: 3 taps
    wide = ResizeCrop((20, 2800))
    wide.check_cap(40, 2800, 4)                                                 # 5 * 2800 * 4 bytes
    with pytest.raises(ValueError, match="intermediate"):
        wide.check_cap(640, 5600, 4)                                            # 65 * 2800 * 4 bytes
    with pytest.raises(ValueError, match="intermediate"):
        ImagePreprocess([0.5] * 4, [0.5] * 4, resize=wide).check([np.zeros((640, 5600, 4), np.uint8)])


def test_plain_preprocess_still_refuses_a_list():
    pre = ImagePreprocess(*IMAGENET)
    ok = np.zeros((2, 4, 4, 3), np.uint8)
    assert pre.resize is None and pre.check(ok) == (2, 3, 4, 4)
    for bad in (list(ok), tuple(ok), [ok]):
        with pytest.raises(ValueError):
            pre.check(bad)
        with pytest.raises(ValueError):
            pre.reference(bad)
    with pytest.raises(ValueError, match="no resize"):
        pre.pack(list(ok))
