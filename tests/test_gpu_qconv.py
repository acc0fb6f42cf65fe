"""GPU: the Conv in integers (QModel.integer_conv) — nqk_im2col_q, tensor.qconv2d, nqk_embed_qi8,
the model flag, the fused plan and the other entry points — against the NumPy restatement
tests/_qconv_ref.py, bit for bit."""
import os
import struct

import numpy as np
import pytest

import _qconv_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
IMAGENET = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])

PADDED = dict(xs=(2, 3, 7, 9), ws=(4, 3, 3, 2), pads=(0, 2, 2, 1), strides=(2, 1))
PATCH = dict(xs=(2, 3, 32, 48), ws=(64, 3, 16, 16), pads=(0, 0, 0, 0), strides=(16, 16))


def _qrange(bw):
    return -(1 << (bw - 1)), (1 << (bw - 1))


def _zp(z):
    return None if z is None else np.int64(z)


# ----------------------------------------------------------------------------- nqk_im2col_q
@pytest.mark.parametrize("dtype", [np.int8, np.int64])
@pytest.mark.parametrize("zx", [None, -7, 127])
def test_im2col_q(dtype, zx):
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    x = np.random.default_rng(1).integers(-128, 128, size=PADDED["xs"], dtype=np.int64)
    cols, rs, ho, wo = K.im2col_q(DeviceArray.from_host(x.astype(dtype)), 3, 2, PADDED["pads"], PADDED["strides"],
                                  pad=0 if zx is None else zx, rowsum=True)
    want, rho, rwo = R.im2col_q(x, 3, 2, PADDED["pads"], PADDED["strides"], zx)
    assert (ho, wo) == (rho, rwo) and cols.dtype == np.dtype(dtype)
    got = cols.to_host()
    np.testing.assert_array_equal(got.astype(np.int64), want)
    np.testing.assert_array_equal(got[0].astype(np.int64), np.full(18, 0 if zx is None else zx))  # all padding
    np.testing.assert_array_equal(rs.to_host(), want.sum(1))
    none = K.im2col_q(DeviceArray.from_host(x.astype(dtype)), 3, 2, PADDED["pads"], PADDED["strides"],
                      pad=0 if zx is None else zx)
    assert none[1] is None
    np.testing.assert_array_equal(none[0].to_host(), got)


def test_im2col_q_refuses():
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    x = DeviceArray.from_host(np.zeros((1, 1, 4, 4), np.int8))
    with pytest.raises(ValueError, match="does not fit"):
        K.im2col_q(x, 2, 2, (0, 0, 0, 0), (1, 1), pad=128)
    with pytest.raises(ValueError, match="dtype"):
        K.im2col_q(DeviceArray.from_host(np.zeros((1, 1, 4, 4), np.float32)), 2, 2, (0, 0, 0, 0), (1, 1))
    with pytest.raises(ValueError, match="strides"):
        K.im2col_q(x, 2, 2, (0, 0, 0, 0), (0, 1))


# ----------------------------------------------------------------------------- qconv2d
@pytest.mark.parametrize("case", [PADDED, PATCH], ids=["padded", "patchify"])
@pytest.mark.parametrize("bw", [8, 4, 12])
@pytest.mark.parametrize("zx,zw", [(None, None), (-3, None), (-3, 2)])
def test_qconv2d(case, bw, zx, zw):
    from numpy_quant.tensor import FTensor, QTensor, qconv2d
    rng = np.random.default_rng(bw)
    lo, hi = _qrange(bw)
    xq = rng.integers(lo, hi, size=case["xs"], dtype=np.int64)
    wq = rng.integers(lo, hi, size=case["ws"], dtype=np.int64)
    sx, sw = np.float32(0.0371), np.float32(0.0042)
    bias = rng.standard_normal(case["ws"][0]).astype(np.float32)
    got = qconv2d(QTensor(xq, bw, sx, _zp(zx)), QTensor(wq, bw, sw, _zp(zw)), FTensor(bias), case["pads"],
                  case["strides"])
    want = R.qconv2d(xq, zx, sx, wq, zw, sw, bias, case["pads"], case["strides"])
    assert got.dev.shape == want.shape
    np.testing.assert_array_equal(got.data, want)


# ----------------------------------------------------------------------------- nqk_embed_qi8
def _embed_case(images, h, w, n_out, rng, zx, xq=None, wq=None, wrange=(-128, 128), l1=None):
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    hw = (h // 16) * (w // 16)
    xq = rng.integers(-128, 128, size=(images, 3, h, w), dtype=np.int64) if xq is None else xq
    wq = rng.integers(*wrange, size=(n_out, 3, 16, 16), dtype=np.int64) if wq is None else wq
    sx, sw = np.float32(0.0187), np.float32(0.0021)
    bias = rng.standard_normal(n_out).astype(np.float32)
    cls = rng.standard_normal(n_out).astype(np.float32)
    pos = rng.standard_normal((hw + 1, n_out)).astype(np.float32)
    wm = wq.reshape(n_out, -1)
    colterm = (wm.sum(1) * (0 if zx is None else zx)).astype(np.int32)
    out = DeviceArray((images, hw + 1, n_out), np.float32)
    K.embed_qi8(DeviceArray.from_host(xq.astype(np.int8)), DeviceArray.from_host(wm.astype(np.int8)),
                DeviceArray.from_host(colterm), np.float32(sx * sw), zx,
                int(np.abs(wm).sum(1).max()) if l1 is None else l1, DeviceArray.from_host(bias),
                DeviceArray.from_host(cls), DeviceArray.from_host(pos), out)
    got = out.to_host()
    want = R.embed(xq, zx, sx, wq, sw, bias, cls, pos)
    np.testing.assert_array_equal(got[:, 0], np.broadcast_to(cls + pos[0], (images, n_out)))
    np.testing.assert_array_equal(got, want)
    return got


@pytest.mark.parametrize("n_out", [64, 192])
@pytest.mark.parametrize("zx", [None, -7])
def test_embed_qi8_ragged_tile_over_three_images(n_out, zx):
    """3 images of 32 x 48: hw = 6, 18 rows — one ragged row tile that spans three images, so the
    + 1 class-row offset changes inside a tile."""
    _embed_case(3, 32, 48, n_out, np.random.default_rng(n_out), zx)


@pytest.mark.parametrize("n_out", [128, 192])
def test_embed_qi8_crosses_a_row_tile(n_out):
    """5 images of 80 x 96: hw = 30, 150 rows — crosses a 128-row tile (and the 64-row wave tiles)."""
    _embed_case(5, 80, 96, n_out, np.random.default_rng(5), -7)


@pytest.mark.parametrize("zx", [-128, 127])
def test_embed_qi8_extreme_operands(zx):
    """All -128 image and weights: the largest accumulator (768 * 2^14) and, at zx = 127, the
    largest correction; |acc - colterm| = 768 * 128 * 255 > 2^24 there: the f64 product."""
    xq = np.full((3, 3, 32, 48), -128, dtype=np.int64)
    wq = np.full((64, 3, 16, 16), -128, dtype=np.int64)
    _embed_case(3, 32, 48, 64, np.random.default_rng(2), zx, xq=xq, wq=wq)


def test_embed_qi8_int4_weights_and_unproven_bound():
    rng = np.random.default_rng(4)
    a = _embed_case(3, 32, 48, 128, rng, -7, wrange=(-8, 8))
    # the same operands with the bound unknown (w_l1max = -1): the f64 product gives the same bits
    b = _embed_case(3, 32, 48, 128, np.random.default_rng(4), -7, wrange=(-8, 8), l1=-1)
    np.testing.assert_array_equal(a, b)


def test_embed_qi8_refuses_and_launches_nothing():
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray, sync
    lib = _lib.load()
    n, c, h, w, n_out = 2, 3, 32, 48, 64
    hw = 6
    q = DeviceArray.from_host(np.ones((n * c * h * w + 64,), np.int8))
    wt = DeviceArray.from_host(np.ones((n_out * 768 + 64,), np.int8))
    ct = DeviceArray.from_host(np.zeros((n_out + 16,), np.int32))
    f = [DeviceArray.from_host(np.zeros((n_out + 16,), np.float32)) for _ in range(2)]
    pos = DeviceArray.from_host(np.zeros(((hw + 1) * n_out + 16,), np.float32))
    sentinel = np.full((n * (hw + 1) * n_out + 16,), -77.0, np.float32)
    out = DeviceArray.from_host(sentinel)

    def call(q_off=0, wt_off=0, ct_off=0, out_off=0, zx=0, c=c, h=h, w=w, kh=16, kw=16, n_out=n_out):
        return lib.nqk_embed_qi8(q.ptr + q_off, wt.ptr + wt_off, ct.ptr + ct_off, 0.5, zx, -1, f[0].ptr, f[1].ptr,
                                 pos.ptr, out.ptr + out_off, n, c, h, w, kh, kw, n_out)

    refused = {
        "unaligned q": dict(q_off=1), "unaligned wt": dict(wt_off=8), "unaligned colterm": dict(ct_off=4),
        "unaligned out": dict(out_off=4), "kw": dict(kw=8), "kh": dict(kh=8), "w % 16": dict(w=40),
        "h % 16": dict(h=24), "N % 64": dict(n_out=32), "zero point": dict(zx=(1 << 20) + 1),
        "negative zero point": dict(zx=-(1 << 20) - 1), "int32 accumulator": dict(zx=30000),
        "no channels": dict(c=0),
    }
    for what, kw in refused.items():
        assert call(**kw) != 0, what
        assert b"nqk_embed_qi8" in lib.nqk_last_error(), what
    sync()
    np.testing.assert_array_equal(out.to_host(), sentinel)  # nothing was launched
    assert call() == 0
    sync()
    assert not (out.to_host()[:n * (hw + 1) * n_out] == -77.0).any()


# ----------------------------------------------------------------------------- model
def _vit(batch, seed=0, tiny=False):
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True,
                            seed=seed)
    if tiny:
        onnx_proto.redimension(proto, 192, 3, 768)
    if batch != 1:
        onnx_proto.rebatch(proto, batch)
    return Model.from_onnx(proto)


def _conv(qmodel):
    return next(n for n in qmodel.nodes if n.op == "Conv")


def _eager(qmodel, x):
    qmodel.keep_values = True
    try:
        return qmodel([x])[0]
    finally:
        qmodel.keep_values = False


@pytest.mark.parametrize("batch,bw", [(3, 8), (2, 4)])
def test_vit_integer_conv(batch, bw):
    from oracle import nq_oracle as O
    x = np.random.default_rng(batch).standard_normal((batch, 3, 224, 224)).astype(np.float32)
    model = _vit(batch)
    qon = model.quantize([x], bw, integer_conv=True)
    assert qon.integer_conv is True
    eager = _eager(qon, x)
    # the node loop's Conv value is the restatement on the qmodel's own integer tensors
    conv = _conv(qon)
    xt, wt, bt = (i.data for i in conv.inputs)
    bias = O.dequantize(bt.data, bt.scale, bt.zero_point)
    want = R.qconv2d(xt.data, xt.zero_point, xt.scale, wt.data, wt.zero_point, wt.scale, bias,
                     tuple(conv.attrs["pads"]), tuple(conv.attrs["strides"]))
    conv_on = conv.outputs[0].data.data
    np.testing.assert_array_equal(conv_on, want)
    # the fused plan: same logits
    plan = qon.compile()
    assert plan.embeds == 1 and plan.fused == 12
    np.testing.assert_array_equal(qon([x])[0], eager)
    # without the flag: the reference-exact path, equal to a quantize_with twin whose flag is off
    qoff = model.quantize([x], bw)
    twin = model.quantize_with(qoff.quant_params, bw, integer_conv=False)
    assert qoff.integer_conv is False and twin.integer_conv is False
    off = qoff([x])[0]
    np.testing.assert_array_equal(twin([x])[0], off)
    np.testing.assert_array_equal(_eager(twin, x), off)
    conv_off = _conv(twin).outputs[0].data.data
    assert conv_off.shape == conv_on.shape and (conv_off != conv_on).any()  # the integer path was taken


# ----------------------------------------------------------------------------- other entry points (ViT-Tiny)
@pytest.fixture(scope="module")
def tiny():
    rng = np.random.default_rng(21)
    u8 = rng.integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    from numpy_quant.images import ImagePreprocess
    pre = ImagePreprocess(*IMAGENET)
    x = pre.reference(u8)
    model = _vit(2, tiny=True)
    qon = model.quantize([x], 8, integer_conv=True)
    return model, qon, pre, u8, x, qon([x])[0]


def test_tiny_plan_equals_eager(tiny):
    model, qon, pre, u8, x, plain = tiny
    assert qon._plan is not None and qon._plan.embeds == 1
    np.testing.assert_array_equal(_eager(qon, x), plain)


def test_tiny_graph_replay(tiny):
    model, qon, pre, u8, x, plain = tiny
    g = qon.graph([x])
    try:
        np.testing.assert_array_equal(g([x])[0], plain)
        np.testing.assert_array_equal(g([x[::-1].copy()])[0], qon([x[::-1].copy()])[0])
    finally:
        g.destroy()


def test_tiny_classify(tiny):
    from numpy_quant.tensor import FTensor
    model, qon, pre, u8, x, plain = tiny
    idx, prob = qon.classify([x], k=5)
    np.testing.assert_array_equal(idx, np.argsort(-plain, axis=-1, kind="stable")[:, :5])
    widx, wprob = FTensor(plain).topk(5)
    np.testing.assert_array_equal(idx, widx.data)
    np.testing.assert_array_equal(prob, wprob.data)


def test_tiny_uint8_images(tiny):
    model, qon, pre, u8, x, plain = tiny
    qon.image_preprocess = pre
    try:
        np.testing.assert_array_equal(qon([u8])[0], plain)
    finally:
        qon.image_preprocess = None


def test_tiny_blob(tiny, tmp_path):
    from numpy_quant import blob
    model, qon, pre, u8, x, plain = tiny
    path = tmp_path / "on.nqk"
    qon.save(path)
    q2 = _vit(2, seed=99, tiny=True).load_quantized(path)
    assert q2.integer_conv is True
    np.testing.assert_array_equal(q2([x])[0], plain)
    assert blob.read(path)[0]["integer_conv"] is True
    # flag off: no key, the bytes of a header that never knew the key, and False on load
    qoff = model.quantize_with(qon.quant_params, 8)
    poff = tmp_path / "off.nqk"
    qoff.save(poff)
    header, _ = blob.read(poff)
    assert "integer_conv" not in header
    raw = open(poff, "rb").read()
    (hl,) = struct.unpack("<Q", raw[8:16])
    assert raw[:8] == blob.MAGIC and raw[16:16 + hl] == blob.encode_header(header)
    known = {"version", "bit_width", "qparams", "constants", "payload_bytes"}
    assert set(header) == known
    q3 = _vit(2, seed=99, tiny=True).load_quantized(poff)
    assert q3.integer_conv is False
    np.testing.assert_array_equal(q3([x])[0], qoff([x])[0])
