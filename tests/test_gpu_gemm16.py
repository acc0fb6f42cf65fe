"""nqk_qgemm_i16 (9..16-bit activations as two byte planes on the int8 MFMAs) against
a.astype(int64) @ b.astype(int64): the entry called directly, the route through QTensor.matmul,
and the encoder layer at (16, 8) and (16, 16) against the NumPy restatement (tests/_mixed_ref.py)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import _mixed_ref as R
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
FILL = -7777777777  # what c holds before a call


def _gemm16(a, bt, ldc=None, bmap=None, bt_code=None, a_off=0, K=None):
    """One nqk_qgemm_i16 call on a [batch][M][K] and bt [nb][N][K]; returns c [batch][M][ldc], pre-filled."""
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray, dtype_code
    batch, M, Ka = a.shape
    N = bt.shape[1]
    K, ldc = K or Ka, ldc or N
    ad, bd = DeviceArray.from_host(a), DeviceArray.from_host(bt)
    cd = DeviceArray.from_host(np.full((batch, M, ldc), FILL, np.int64))
    _lib.call("nqk_qgemm_i16", ctypes.c_void_p(ad.ptr + a_off), bd.vp, dtype_code(bt.dtype) if bt_code is None else bt_code,
              cd.vp, batch, M, N, K, Ka, Ka, ldc, _lib.i64arr(bmap) if bmap else None, M * Ka, N * Ka, M * ldc)
    return cd.to_host()


CASES = [((37, 50, 80), "random"), ((129, 130, 64), "random"), ((16, 16, 4096), "random"), ((16, 16, 65520), "random"),
         ((37, 50, 80), "low-plane"), ((37, 50, 80), "high-plane"), ((16, 16, 4096), "min"), ((16, 16, 65520), "min"),
         ((16, 16, 65520), "max")]


@pytest.mark.parametrize("bdt", [np.int8, np.int16], ids=["b8", "b16"])
@pytest.mark.parametrize("shape,fill", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{f}" for s, f in CASES])
def test_entry_equals_the_int64_product(shape, fill, bdt):
    M, N, K = shape
    rng = np.random.default_rng(M + N + K)
    lo, hi = np.iinfo(bdt).min, np.iinfo(bdt).max
    if fill == "min":  # K = 4096: 2^34 and 2^42; K = 65520 at int16: every plane product 2^14, the cross sum 65520 * 2^15
        a, bt = np.full((M, K), -32768, np.int16), np.full((N, K), lo, bdt)
    elif fill == "max":
        a, bt = np.full((M, K), 32767, np.int16), np.full((N, K), hi, bdt)
    else:
        a = rng.integers(-32768, 32768, size=(M, K)).astype(np.int16)
        bt = rng.integers(lo, hi + 1, size=(N, K)).astype(bdt)
        a[0, :2], a[-1, -2:], bt[0, :2], bt[-1, -2:] = (-32768, 32767), (32767, -32768), (lo, hi), (hi, lo)
        assert a.min() == -32768 and a.max() == 32767 and bt.min() == lo and bt.max() == hi
        if fill == "low-plane":  # only the low byte varies, around its flipped top bit
            a = rng.choice(np.array([0x0080, 0x007F, 0x00FF, 0x0000], np.int16), size=(M, K))
        elif fill == "high-plane":
            a = (a & ~np.int16(255)).astype(np.int16)
    want = a.astype(np.int64) @ bt.astype(np.int64).T
    if fill == "min" and K == 4096:
        assert want[0, 0] == (1 << 34 if bdt == np.int8 else 1 << 42)
    assert np.array_equal(_gemm16(a[None], bt[None])[0], want)


def test_entry_batch_with_a_shared_b_and_a_wide_ldc():
    rng = np.random.default_rng(3)
    a = rng.integers(-32768, 32768, size=(3, 37, 80)).astype(np.int16)
    for bdt in (np.int8, np.int16):
        bt = rng.integers(np.iinfo(bdt).min, np.iinfo(bdt).max + 1, size=(1, 50, 80)).astype(bdt)
        want = np.full((3, 37, 56), FILL, np.int64)
        want[:, :, :50] = a.astype(np.int64) @ bt[0].astype(np.int64).T
        assert np.array_equal(_gemm16(a, bt, ldc=56, bmap=[1, 1, 0, 0, 0]), want)


def test_entry_refuses_before_it_launches():
    from numpy_quant._lib import NQKError
    from numpy_quant.device import dtype_code
    a, bt = np.ones((1, 16, 65536), np.int16), np.ones((1, 16, 65536), np.int8)
    with pytest.raises(NQKError, match="65536"):
        _gemm16(a, bt)
    for kw, msg in ((dict(a_off=2, K=64), "aligned"), (dict(bt_code=dtype_code(np.dtype(np.int32))), "bt_dtype")):
        with pytest.raises(NQKError, match=msg):
            _gemm16(a[:, :, :80].copy(), bt[:, :, :80].copy(), **kw)


# ----------------------------------------------------------------------------- the route
@pytest.mark.parametrize("shape", [(37, 80, 50), (37, 77, 50), (5, 16, 7)], ids=["mfma", "mfma-padded-K", "generic"])
@pytest.mark.parametrize("bits,wbits", [(16, 8), (16, 16), (12, 8), (12, 12)])
def test_matmul_of_a_wide_activation_takes_the_byte_plane_kernel(shape, bits, wbits, monkeypatch):
    from numpy_quant import kernels as K
    from numpy_quant.tensor import FTensor, quantize_tensor
    M, Kd, N = shape
    rng = np.random.default_rng(100 * bits + wbits + Kd)
    xf = rng.standard_normal((M, Kd)).astype(np.float32)
    wf = rng.standard_normal((Kd, N)).astype(np.float32)
    wf[0, 0] = np.float32(-1.5) * wf.max()  # past the symmetric range's low end: both ends of the width are reached
    s_x, zp_x = O.quant_parameters(xf.min(), xf.max(), bits, True)
    s_w, _ = O.quant_parameters(*R.weight_range(wf), wbits, False)
    xq, wq = O.quantize(xf, bits, s_x, zp_x), O.quantize(wf, wbits, s_w, None)
    assert (xq.min(), xq.max()) == tuple(O.qrange(bits)) and (wq.min(), wq.max()) == tuple(O.qrange(wbits))
    acc, s, z = O.q_matmul(xq, s_x, zp_x, wq, s_w, None)
    x = quantize_tensor(FTensor(xf), bits, s_x, zp_x)
    w = quantize_tensor(FTensor(wf), wbits, s_w, None)
    assert x.dev.dtype == np.int16 and np.array_equal(x.data, xq) and np.array_equal(w.data, wq)
    w._is_weight = wbits < bits  # the narrow one is a weight (its Bt is cached); the equal one any tensor
    outs = []
    for leg in ("1", "0"):
        monkeypatch.setenv("NQK_GEMM16", leg)
        monkeypatch.setattr(K, "TIMER", K.KernelTimer())
        out = x.matmul(w)
        assert out.bit_width == 4 * bits and out.dev.dtype == np.int64
        assert np.array_equal(out.data, acc)
        tags = [r[0] for r in K.TIMER.collect()]
        assert tags == (["qgemm_i16"] if leg == "1" and shape[0] > 5 else []), tags
        assert np.array_equal(np.asarray(out.scale, np.float32).view(np.uint32), np.asarray(s, np.float32).view(np.uint32))
        assert np.array_equal(np.broadcast_to(out.zero_point, acc.shape), np.broadcast_to(z, acc.shape))
        outs.append(out.dequantize().data)
        assert np.array_equal(outs[-1].view(np.uint32), O.dequantize(acc, s, z).view(np.uint32))
    assert outs[0].tobytes() == outs[1].tobytes()


# ----------------------------------------------------------------------------- the model
@pytest.mark.parametrize("wbw", [8, 16])
def test_encoder_layer_at_16_bits_equals_the_restatement(wbw, monkeypatch):
    """The encoder-layer fixture itself at batch 1 (the restatement takes about a second on the host)."""
    from numpy_quant import kernels as K
    from numpy_quant.model import Model
    proto, graph, x = R.encoder_layer_fixture(MODELS, batch=1)
    qp, qc, axes = R.calibrate(graph, [x], 16, wbw)
    want = R.outputs_of(graph, R.quantized_forward(graph, qp, qc, [x], 16, weights=axes))
    qmodel = Model.from_onnx(proto).quantize([x], bit_width=16, weight_bit_width=wbw)
    monkeypatch.setattr(K, "TIMER", K.KernelTimer())
    got = qmodel([x])
    products = sum(op in ("MatMul", "Gemm") for _, op, *_ in graph.nodes)
    assert products >= 6 and sum(r[0] == "qgemm_i16" for r in K.TIMER.collect()) == products  # none left on the generic kernel
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32), w.view(np.uint32))
