"""CPU: the host definition of uint8 image inputs (numpy_quant/images.py).  normalize and
quantize are elementwise per channel, so both are a 256-entry table lookup per channel:
every comparison is bit-exact (floats compared as uint32)."""
import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from numpy_quant.images import ImagePreprocess
from oracle import nq_oracle as O

IMAGENET = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
PARAMS = {
    1: [([0.5], [0.5]), ([0.1307], [0.3081]), ([-0.37], [1.73])],
    3: [IMAGENET, ([0.5] * 3, [0.5] * 3), ([0.11, -2.3, 7.0], [0.013, 3.7, -0.9])],
    4: [([0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.5]), ([0.5] * 4, [0.5] * 4),
        ([0.3, 1e-3, -5.5, 0.77], [1.9, 0.07, 2.0 / 3.0, 11.0])],
}
CASES = [(c, mean, std) for c in (1, 3, 4) for mean, std in PARAMS[c]]


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def images(c, layout, seed=0, n=2, h=5, w=130):
    """every (channel, value) pair 0..255 appears: w * h * n >= 256 and a ramp in front"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    img.reshape(-1, c)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    return img if layout == "NHWC" else np.ascontiguousarray(img.transpose(0, 3, 1, 2))


def gather(table, img, layout):
    """table[c][img[..., c]] as NCHW"""
    c = table.shape[0]
    nchw = img.transpose(0, 3, 1, 2) if layout == "NHWC" else img
    return np.ascontiguousarray(np.stack([table[ci][nchw[:, ci]] for ci in range(c)], axis=1))


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("c,mean,std", CASES)
def test_reference_is_the_written_formula(c, mean, std, layout):
    pre = ImagePreprocess(mean, std, layout=layout)
    img = images(c, layout)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    nhwc = img if layout == "NHWC" else img.transpose(0, 2, 3, 1)
    want = np.empty(nhwc.shape, np.float32)
    for ci in range(c):
        x = nhwc[..., ci].astype(np.float32) / np.float32(255)
        want[..., ci] = (x - m[ci]) / s[ci]
    want = np.ascontiguousarray(want.transpose(0, 3, 1, 2))
    got = pre.reference(img)
    assert got.dtype == np.float32 and got.flags.c_contiguous and got.shape == want.shape
    np.testing.assert_array_equal(bits(got), bits(want))


def test_rescale_is_used():
    pre = ImagePreprocess([0.0], [1.0], rescale=1)
    img = images(1, "NHWC")
    np.testing.assert_array_equal(bits(pre.reference(img)), bits(img.transpose(0, 3, 1, 2).astype(np.float32)))


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("c,mean,std", CASES)
def test_table_gathered_is_reference(c, mean, std, layout):
    pre = ImagePreprocess(mean, std, layout=layout)
    img = images(c, layout, seed=1)
    table = pre.table()
    assert table.shape == (c, 256) and table.dtype == np.float32
    np.testing.assert_array_equal(bits(gather(table, img, layout)), bits(pre.reference(img)))


@pytest.mark.parametrize("bw", [4, 8, 16])
@pytest.mark.parametrize("c,mean,std", CASES)
def test_quantized_table_gathered_is_quantized_reference(c, mean, std, bw):
    pre = ImagePreprocess(mean, std)
    img = images(c, "NHWC", seed=2)
    ref = pre.reference(img)
    asym = O.quant_parameters(ref.min(), ref.max(), bw, True)
    sym = O.quant_parameters(ref.min(), ref.max(), bw, False)
    odd = (np.float32(0.0123), np.array(-3, dtype=np.int64))
    for scale, zp in (asym, sym, odd):
        lut = O.quantize(pre.table(), bw, scale, zp)
        np.testing.assert_array_equal(gather(lut, img, "NHWC"), O.quantize(ref, bw, scale, zp))


def test_validation_errors():
    pre = ImagePreprocess(*IMAGENET)
    ok = np.zeros((2, 4, 4, 3), np.uint8)
    assert pre.check(ok) == (2, 3, 4, 4)
    for bad in (ok.astype(np.float32), ok.astype(np.int8), ok[0], ok[..., :2], ok[:0], np.zeros((2, 0, 4, 3), np.uint8),
                [[1, 2, 3]]):
        with pytest.raises(ValueError):
            pre.check(bad)
        with pytest.raises(ValueError):
            pre.reference(bad)
    chw = ImagePreprocess(*IMAGENET, layout="NCHW")
    assert chw.check(np.zeros((2, 3, 4, 5), np.uint8)) == (2, 3, 4, 5)
    with pytest.raises(ValueError):
        chw.check(ok)  # channels last in an NCHW preprocess


@pytest.mark.parametrize("mean,std,kw", [
    ([0.5] * 3, [0.5, 0.0, 0.5], {}), ([0.5], [np.inf], {}), ([0.5], [np.nan], {}), ([0.5] * 5, [0.5] * 5, {}),
    ([], [], {}), ([0.5] * 3, [0.5] * 2, {}), ([0.5], [0.5], {"layout": "HWC"}), ([0.5], [0.5], {"rescale": 0}),
])
def test_constructor_errors(mean, std, kw):
    with pytest.raises(ValueError):
        ImagePreprocess(mean, std, **kw)
