"""The float GEMM family (nqk_sgemm: k_sgemm_blas, the three k_sgemm_mfma forms, k_sgemm_small;
nqk_sgemm_embed; the k_embed_q forms; kernels.matmul_f32, model._gemm, tensor.fconv2d) against
tests/_sgemm_ref.py, the host-independent restatement of np.matmul that
tests/test_sgemm_ref_host.py pins to NumPy — never against the GPU host's own BLAS.  Bit for bit
as int32 views, any NaN equal to any NaN.  The kernel a case runs follows from the launcher's
conditions (nqk_gemm.hip nqk_sgemm), which the case ids restate; no call reports it."""
import numpy as np
import pytest

import _sgemm_ref as R

pytestmark = pytest.mark.gpu

_REF = {}


def _case(M, N, K, transb, threads, seed=0):
    """Operands with the edge values at the ragged tile's last rows and columns and around every
    K-block boundary, and their reference; computed once per case."""
    key = (M, N, K, transb, threads, seed)
    if key not in _REF:
        level3 = R.gemm_regime(M, N, K, transb) == "level3"
        blocks = R.k_blocks(K, R.gemm_driver(M, N, K, threads)) if level3 else [K]
        a, b = R.edge_operands(M, N, K, 7 * M + 3 * N + K + seed, blocks)
        want = R.sgemm_ref(a, b, transb, threads)
        for arr in (a, b, want):
            arr.setflags(write=False)
        _REF[key] = (a, b, want)
    return _REF[key]


def _assert_same(got, want, what=""):
    same = R.same_bits(got, want)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} differ, first at {np.argwhere(~same)[:4].tolist()}"


def _edge_values_present(want):
    assert np.isnan(want).any() and np.isinf(want).any()
    mag = np.abs(want[np.isfinite(want)])
    assert ((mag > 0) & (mag < np.finfo(np.float32).tiny)).any()


# (id, M, N, K, threads, environment): the kernel the launcher takes under these conditions
_ROUTES = [
    # k_sgemm_blas: an odd K; an odd block end inside an even K (threaded 225 + 225); the switch; M N < 128^2
    ("blas-oddK-449", 129, 131, 449, 8, {}),
    ("blas-oddend-450", 129, 131, 450, 8, {}),
    ("blas-oddend-898", 129, 131, 898, 8, {}),
    ("blas-3blocks-1345", 304, 131, 1345, 8, {}),
    ("blas-switch-452", 129, 131, 452, 8, {"NQK_SGEMM_VALU": "1"}),
    ("blas-smallMN-452", 100, 131, 452, 8, {}),
    # k_sgemm_mfma<.., false>: block ends inside a 16-k tile (226; single driver 240 + 210 of K = 450)
    ("mfma-tile-452", 129, 131, 452, 8, {}),
    ("mfma-single-450", 129, 131, 450, 1, {}),
    ("mfma-single-898", 129, 132, 898, 1, {}),
    ("mfma-al16off-896", 129, 132, 896, 8, {"NQK_SGEMM_AL16": "0"}),
    # k_sgemm_mfma<.., true, true> and <.., true>: block ends at the end of a 16-k tile
    ("mfma-vec-896", 129, 132, 896, 8, {}),
    ("mfma-scalar-896", 129, 132, 896, 8, {"NQK_SGEMM_SCALAR": "1"}),
    ("mfma-scalar-N131-1344", 257, 131, 1344, 8, {}),
    ("mfma-vec-1344", 130, 128, 1344, 16, {}),
    # k_sgemm_small (at most 10^6 products): column tails of 4 + 2 + 1, 2 and 8, row tails, no K blocking
    ("small-20x100x77", 20, 100, 77, 8, {}),
    ("small-7x23x40", 7, 23, 40, 8, {}),
    ("small-17x18x33", 17, 18, 33, 8, {}),
    ("small-6x24x500", 6, 24, 500, 8, {}),
    ("small-6x17x31", 6, 17, 31, 8, {}),
    ("small-boundary-25x40x1000", 25, 40, 1000, 8, {}),
    ("level3-boundary-25x40x1001", 25, 40, 1001, 8, {}),
    ("level3-single-16x16x3907", 16, 16, 3907, 8, {}),
]


@pytest.mark.parametrize("name,M,N,K,threads,env", _ROUTES, ids=[r[0] for r in _ROUTES])
def test_sgemm_routes_equal_reference(name, M, N, K, threads, env, monkeypatch):
    from numpy_quant import kernels as KM
    from numpy_quant.device import DeviceArray
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(KM, "BLAS_THREADS", threads)
    a, b, want = _case(M, N, K, False, threads)
    assert KM.gemm_restated(M, N, K, False)
    _edge_values_present(want)
    got = KM.sgemm(DeviceArray.from_host(a), K, 1, DeviceArray.from_host(b), N, 1, M, N, K).to_host()
    _assert_same(got, want, name)


@pytest.mark.parametrize("M,N,K", [(6, 7, 64), (16, 16, 1000), (30, 40, 100), (30, 41, 100), (20, 20, 31), (129, 131, 450)])
def test_gemm_op_transb_equals_reference(M, N, K, monkeypatch):
    """The Gemm operator with transB at M >= 2 (model._gemm): the transposed form's small kernels
    (M N <= 1200, K >= 32), read from w as it lies; their refusals and the level-3 regime."""
    from numpy_quant import kernels as KM
    from numpy_quant.model import _gemm
    from numpy_quant.tensor import FTensor
    a, b, want = _case(M, N, K, True, 8)
    assert KM.gemm_restated(M, N, K, True)
    bias = np.random.default_rng(K).standard_normal(N).astype(np.float32)
    w = np.ascontiguousarray(b.T)
    got = _gemm([FTensor(a), FTensor(w), FTensor(bias)], {"transB": 1, "alpha": 1.0, "beta": 1.0})[0].data
    with np.errstate(all="ignore"):
        _assert_same(got, want + bias[None, :])
    # a MatMul fed by a Transpose node is the same BLAS call
    got = FTensor(a).matmul(FTensor(w).transpose([1, 0])).data
    _assert_same(got, want)


@pytest.mark.parametrize("M,N,K", [(7, 23, 40), (40, 60, 450)])
def test_matmul_f32_batch_map_with_broadcast(M, N, K):
    """kernels.matmul_f32 over a batch map with a broadcast operand on each side, (2, 1, M, K) @
    (1, 2, K, N): NumPy calls BLAS once per matrix, so every matrix is in its own regime."""
    from numpy_quant import kernels as KM
    from numpy_quant.device import DeviceArray
    ops = [_case(M, N, K, False, 8, seed) for seed in (0, 1)]
    a = np.stack([ops[0][0], ops[1][0]])[:, None]
    b = np.stack([ops[0][1], ops[1][1]])[None, :]
    got = KM.matmul_f32(DeviceArray.from_host(a), DeviceArray.from_host(b)).to_host()
    assert got.shape == (2, 2, M, N)
    for i in range(2):
        for j in range(2):
            want = ops[i][2] if i == j else R.sgemm_ref(a[i, 0], b[0, j], False, 8)
            _assert_same(got[i, j], want, f"matrix {i},{j}")


def _im2col(x, kh, kw, pads, strides):
    n, c, h, w = x.shape
    xp = np.zeros((n, c, h + pads[0] + pads[2], w + pads[1] + pads[3]), np.float32)
    xp[:, :, pads[0]:pads[0] + h, pads[1]:pads[1] + w] = x
    ho = (xp.shape[2] - kh) // strides[0] + 1
    wo = (xp.shape[3] - kw) // strides[1] + 1
    cols = np.zeros((n, ho, wo, kh, kw, c), np.float32)
    for i in range(ho):
        for j in range(wo):
            cols[:, i, j] = xp[:, :, i * strides[0]:i * strides[0] + kh, j * strides[1]:j * strides[1] + kw].transpose(0, 2, 3, 1)
    return cols.reshape(n * ho * wo, kh * kw * c), ho, wo


@pytest.mark.parametrize("xs,ws,pads,strides", [((1, 4, 9, 11), (5, 4, 3, 3), (1, 1, 1, 1), (2, 2)),
                                                ((1, 3, 32, 48), (64, 3, 16, 16), (0, 0, 0, 0), (16, 16)),
                                                ((3, 3, 40, 40), (20, 3, 7, 7), (2, 3, 2, 3), (3, 2))])
def test_fconv2d_equals_reference(xs, ws, pads, strides):
    """tensor.fconv2d with padding and stride: the reference's sliding windows, x.dot(w) on two
    contiguous matrices and the bias add.  30 x 5 x 36 (a 4 + 1 column tail of dot products, a row
    tail), the 32 x 48 image's patch embedding 6 x 64 x 768 (small regime: one chain over K = 768,
    no 384 + 384 blocks), and 780 x 20 x 147 in the level-3 regime."""
    from numpy_quant.tensor import FTensor, fconv2d
    rng = np.random.default_rng(sum(xs) + sum(ws))
    x = rng.standard_normal(xs).astype(np.float32)
    w = rng.standard_normal(ws).astype(np.float32)
    bias = rng.standard_normal(ws[0]).astype(np.float32)
    cols, ho, wo = _im2col(x, ws[2], ws[3], pads, strides)
    wm = np.ascontiguousarray(w.transpose(2, 3, 1, 0)).reshape(-1, ws[0])
    y = R.sgemm_ref(cols, wm, False, 8) + bias[None, :]
    want = y.reshape(xs[0], ho, wo, ws[0]).transpose(0, 3, 1, 2)
    got = fconv2d(FTensor(x), FTensor(w), FTensor(bias), pads, strides).data
    assert got.shape == want.shape
    _assert_same(got, want)


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("mfma", ["32", "16"])
def test_embed_kernels_equal_reference(N, mfma, monkeypatch):
    """nqk_sgemm_embed and nqk_embed_q (both MFMA forms, the 128 x 64 and 128 x 128 tiles): 22 images
    of 32 x 48 (132 patch rows: a full row tile and a ragged one; 132 N 768 > 10^6, the level-3
    regime, K = 768 = 384 + 384 under both drivers) against sgemm_ref of the dequantized patch
    matrix, then the bias and the position embedding in the node loop's order."""
    monkeypatch.setenv("NQK_EMBED_MFMA", mfma)
    from numpy_quant import _lib
    from numpy_quant.device import DeviceArray, permute
    from numpy_quant.plan import embed_weight_image
    n, h, w, zp = 22, 32, 48, -7
    hw = (h // 16) * (w // 16)
    rng = np.random.default_rng(N)
    q = rng.integers(-128, 128, size=(n, 3, h, w), dtype=np.int8)
    s = np.float32(0.0173)
    W = (0.05 * rng.standard_normal((N, 3, 16, 16))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    cls = rng.standard_normal(N).astype(np.float32)
    pos = rng.standard_normal((hw + 1, N)).astype(np.float32)
    x = ((q.astype(np.float32) - np.float32(zp)) * s).astype(np.float32)
    cols, _, _ = _im2col(x, 16, 16, (0, 0, 0, 0), (16, 16))
    wm = np.ascontiguousarray(W.transpose(2, 3, 1, 0)).reshape(768, N)
    assert R.gemm_regime(n * hw, N, 768) == "level3"
    y = (R.sgemm_ref(cols, wm, False, 8) + bias[None, :]).reshape(n, hw, N) + pos[None, 1:, :]
    want = np.concatenate([np.broadcast_to(cls + pos[0], (n, 1, N)), y], axis=1)
    dbias, dcls, dpos = (DeviceArray.from_host(v) for v in (bias, cls, pos))
    Wd = DeviceArray.from_host(W)
    qd = DeviceArray.from_host(q)
    dcols = DeviceArray((n * hw, 768), np.float32)
    _lib.call("nqk_patchify_dequant", qd.vp, dcols.vp, n, 3, h, w, 16, 16, float(s), zp)
    _assert_same(dcols.to_host(), cols, "patch matrix")
    out = DeviceArray((n, hw + 1, N), np.float32)
    dwm = permute(Wd, [2, 3, 1, 0]).reshape((768, N))
    _lib.call("nqk_sgemm_embed", dcols.vp, dwm.vp, dbias.vp, dcls.vp, dpos.vp, out.vp, n, hw, N, 768)
    _assert_same(out.to_host(), want, "nqk_sgemm_embed")
    assert _lib.load().nqk_embed_weight_order() == int(mfma)
    wt = embed_weight_image(Wd, N, 768)
    out2 = DeviceArray((n, hw + 1, N), np.float32)
    _lib.call("nqk_embed_q", qd.vp, float(s), zp, wt.vp, dbias.vp, dcls.vp, dpos.vp, out2.vp, n, 3, h, w, 16, 16, N)
    _assert_same(out2.to_host(), want, "nqk_embed_q")


def test_embed_kernels_refuse_driver_dependent_blocks():
    """nqk_sgemm_embed has no thread count: a K whose blocks the two OpenBLAS drivers cut
    differently (450: 225 + 225 against 240 + 210) is refused, and the plan does not fuse it."""
    from numpy_quant import _lib, kernels as KM
    from numpy_quant.device import DeviceArray
    assert KM.blas_kblocks(450, True) == R.k_blocks(450, "threaded") != R.k_blocks(450, "single") == KM.blas_kblocks(450, False)
    assert KM.blas_kblocks(768, True) == KM.blas_kblocks(768, False) == [384, 384]
    z = DeviceArray.from_host(np.zeros((7 * 450,), np.float32))
    with pytest.raises(_lib.NQKError, match="drivers block alike"):
        _lib.call("nqk_sgemm_embed", z.vp, z.vp, z.vp, z.vp, z.vp, z.vp, 1, 2, 4, 450)


def test_fused_embed_leaves_small_regime_to_the_node_operators():
    """plan.FusedEmbed at one 32 x 48 image and width 64 (6 x 64 x 768 <= 10^6 products: np.matmul's
    small-matrix kernels, one chain over K = 768): the step does not take nqk_embed_q /
    nqk_sgemm_embed, whose order is the level-3 one (384 + 384), and equals the reference."""
    from types import SimpleNamespace as NS
    from numpy_quant import kernels as KM
    from numpy_quant.plan import FusedEmbed
    from numpy_quant.tensor import FTensor, ITensor, QTensor
    n, N, hw = 1, 64, 6
    rng = np.random.default_rng(64)
    xq = QTensor(rng.integers(-128, 128, size=(n, 3, 32, 48), dtype=np.int64), 8, np.float32(0.0173), np.int64(-7))
    x = xq.dequantize().data
    W = rng.standard_normal((N, 3, 16, 16)).astype(np.float32)
    bias, cls = rng.standard_normal(N).astype(np.float32), rng.standard_normal((1, 1, N)).astype(np.float32)
    pos = rng.standard_normal((1, hw + 1, N)).astype(np.float32)
    assert KM.gemm_small_regime(n * hw, N, 768) and R.gemm_regime(n * hw, N, 768) == "small"
    val = lambda a: NS(data=FTensor(a))  # noqa: E731
    m = NS(x=NS(data=xq), w=val(W), b=val(bias), cls=val(cls), pos=val(pos), kh=16, kw=16,
           expand=NS(inputs=[None, NS(data=ITensor(np.array([n, 1, N], dtype=np.int64)))]),
           add=NS(outputs=[NS(data=None)]), conv_out=NS(data=None, name="conv_out"))
    qmodel = NS(_dequant_input=lambda v: v.data.dequantize() if isinstance(v.data, QTensor) else v.data)
    FusedEmbed(qmodel, m).run(qmodel)
    got = m.add.outputs[0].data.data
    cols, _, _ = _im2col(x, 16, 16, (0, 0, 0, 0), (16, 16))
    wm = np.ascontiguousarray(W.transpose(2, 3, 1, 0)).reshape(768, N)
    small = R.sgemm_ref(cols, wm, False, 8)
    level3 = R.blocked_chain(cols, wm, [384, 384])
    assert not R.same_bits(small, level3).all()  # the two orders differ on these operands
    want = np.concatenate([np.broadcast_to(cls, (n, 1, N)), (small + bias[None, :]).reshape(n, hw, N)], axis=1) + pos
    _assert_same(got, want)
