"""tests/_fused_ref.py (the NumPy restatement of the fused kernels that
tests/test_gpu_fused_reference.py compares them with) against the oracle's node loop, on the CPU:
the encoder-layer graph is calibrated and run by oracle/nq_oracle.py (QModel.__call__,
model.py:486-565), the quantized operands and qparams of the layer are taken from its node
values, and every helper function must reproduce the oracle's value at the end of its chain,
bit for bit.  Uses nothing of numpy_quant but the pure-Python ONNX loader."""
import os

import numpy as np
import pytest

import _fused_ref as R
from conftest import ROOT
from oracle import nq_oracle as O

MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
AT = "/attention/attention/"


@pytest.fixture(scope="module")
def layer():
    from numpy_quant import onnx_proto
    path = os.path.join(MODELS, "vit_image_classifier_encoder_layer_no_weights.onnx")
    x = np.random.default_rng(5).standard_normal((1, 197, 768)).astype(np.float32)
    graph = O.Graph(onnx_proto.load(path, synthetic_weights=True))
    with np.errstate(all="ignore"):
        qp, qc = O.calibrate(graph, [x], 8)
        vals = O.quantized_forward(graph, qp, qc, [x], 8)
    return graph, qp, qc, vals


@pytest.fixture(scope="module")
def layer226():
    """The same graph re-dimensioned to ViT-Ti (192 wide, 3 heads) and re-tokened to 226 (240 px):
    past nqk_attention_fused's 224 tokens, where tests/test_gpu_attention_long_reference.py rests
    on this reference."""
    from numpy_quant import onnx_proto
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_encoder_layer_no_weights.onnx"), synthetic_weights=True)
    assert onnx_proto.redimension(proto, 192, 3, 768) > 0
    assert onnx_proto.retoken(proto, 226) == 6
    x = np.random.default_rng(226).standard_normal((1, 226, 192)).astype(np.float32)
    graph = O.Graph(proto)
    with np.errstate(all="ignore"):
        qp, qc = O.calibrate(graph, [x], 8)
        vals = O.quantized_forward(graph, qp, qc, [x], 8)
    return graph, qp, qc, vals


def _q(layer, name):
    """The quantized operand the oracle's MatMul makes of float value `name` (int64), its scale
    and zero point."""
    _, qp, _, vals = layer
    t = vals[name]
    p = qp[name]
    if t[0] == "Q":
        return t[1], np.float32(t[3]), t[4]
    return O.quantize(t[1], 8, p.scale, p.zero_point), np.float32(p.scale), p.zero_point


def _w(layer, name):
    """A weight constant as bt [N][K] int8 and its scale (symmetric: no zero point)."""
    t = layer[2][name]
    assert t[4] is None
    return np.ascontiguousarray(t[1].T).astype(np.int8), np.float32(t[3])


def _bias(layer, name):
    return O.q_dequant(layer[2][name])[1]


def _i8(a):
    assert a.min() >= -128 and a.max() <= 127
    return a.astype(np.int8)


def test_qkv_matches_oracle(layer):
    a, s_a, zpa = _q(layer, "/layernorm_before/LayerNormalization_output_0")
    ws = [_w(layer, n) for n in ("onnx::MatMul_106", "onnx::MatMul_107", "onnx::MatMul_113")]
    bt = np.concatenate([w for w, _ in ws])
    bias = np.concatenate([_bias(layer, f"attention.attention.{n}.bias") for n in ("query", "key", "value")])
    outs = [AT + "Transpose_1_output_0", AT + "Transpose_2_output_0", AT + "Transpose_output_0"]
    tq = [_q(layer, n) for n in outs]
    got = R.qkv(_i8(a[0]), bt, bias, int(zpa), [s_a * s for _, s in ws], [t[1] for t in tq], [int(t[2]) for t in tq], 8,
                197, 12, 64)
    want_q, want_k, want_v = tq[0][0][0], tq[1][0][0].transpose(0, 2, 1), tq[2][0][0]  # [H, T, Dh]
    for g, w in zip(got, (want_q, want_k, want_v)):
        np.testing.assert_array_equal(g.reshape(12, 197, 64).astype(np.int64), w)


def _attention_operands(layer):
    q, s_q, zq = _q(layer, AT + "Transpose_1_output_0")
    kt, s_k, zk = _q(layer, AT + "Transpose_2_output_0")
    v, s_v, zv = _q(layer, AT + "Transpose_output_0")
    return _i8(q[0]), _i8(kt[0].transpose(0, 2, 1)), _i8(v[0]), (s_q, int(zq)), (s_k, int(zk)), (s_v, int(zv))


def _check_scores_softmax_context(layer, T, heads):
    _, qp, _, vals = layer
    Tp = (T + 15) // 16 * 16
    q, k, v, (s_q, zq), (s_k, zk), (s_v, zv) = _attention_operands(layer)
    div = vals[AT + "Constant_3_output_0"][1]
    assert div.shape == () and float(div) == 8.0
    s = R.scores(q, k, zq, zk, s_q * s_k, float(div))
    np.testing.assert_array_equal(s.view(np.int32), vals[AT + "Div_output_0"][1][0].view(np.int32))
    pq, s_p, zp_p = _q(layer, AT + "Softmax_output_0")
    p, rows = R.softmax_quant(s, Tp, s_p, int(zp_p), 8)
    np.testing.assert_array_equal(p[..., :T].astype(np.int64), pq[0])
    assert not p[..., T:].any()
    np.testing.assert_array_equal(rows, pq[0].sum(axis=-1))
    cq, s_c, zc = _q(layer, AT + "Reshape_3_output_0")
    ctx = R.pv(p, v, int(zp_p), zv, s_p * s_v, s_c, int(zc), 8, heads, T)
    np.testing.assert_array_equal(ctx.astype(np.int64), cq)
    # the composition, and the transpose helper on V
    np.testing.assert_array_equal(R.attention(q, k, v, heads, zq, zk, s_q * s_k, float(div), s_p, int(zp_p), s_p * s_v, zv,
                                              s_c, int(zc), 8), ctx)
    vt, vsum = R.transpose_pad(v, Tp)
    np.testing.assert_array_equal(vt[:, :, :T], v.transpose(0, 2, 1))
    assert not vt[:, :, T:].any()
    np.testing.assert_array_equal(vsum, v.astype(np.int64).sum(axis=1))
    return q.shape


def test_scores_softmax_context_match_oracle(layer):
    assert _check_scores_softmax_context(layer, 197, 12) == (12, 197, 64)


def test_scores_softmax_context_match_oracle_at_226_tokens(layer226):
    """Rows of 226 scores (Tp = 240): the reference of the long-sequence attention tests rests on
    the oracle's node loop, not on itself."""
    assert _check_scores_softmax_context(layer226, 226, 3) == (3, 226, 64)


def test_residual_sums_match_oracle(layer):
    _, qp, _, vals = layer
    a, s_a, zpa = _q(layer, AT + "Reshape_3_output_0")
    bt, s_w = _w(layer, "onnx::MatMul_128")
    x0 = O.q_dequant(vals["inputs"])[1][0]
    y1 = R.resid(_i8(a[0]), bt, _bias(layer, "attention.output.dense.bias"), x0, int(zpa), s_a * s_w)
    np.testing.assert_array_equal(y1.view(np.int32), vals["/Add_output_0"][1][0].view(np.int32))
    a2, s_a2, zpa2 = _q(layer, "/intermediate/intermediate_act_fn/Mul_1_output_0")
    bt2, s_w2 = _w(layer, "onnx::MatMul_130")
    y2 = R.resid(_i8(a2[0]), bt2, _bias(layer, "output.dense.bias"), y1, int(zpa2), s_a2 * s_w2)
    np.testing.assert_array_equal(y2.view(np.int32), vals["hidden_states"][1][0].view(np.int32))
    # the fused-LayerNorm form: the oracle's second LayerNorm of the first residual sum, quantized
    # for its consumer MatMul
    ln, s_ln, zp_ln = _q(layer, "/layernorm_after/LayerNormalization_output_0")
    g, b = vals["layernorm_after.weight"], vals["layernorm_after.bias"]
    g, b = (O.q_dequant(t)[1] if t[0] == "Q" else t[1] for t in (g, b))
    rows, lnq = R.resid_ln(_i8(a[0]), bt, _bias(layer, "attention.output.dense.bias"), x0, int(zpa), s_a * s_w, g, b,
                           9.999999960041972e-13, s_ln, int(zp_ln), 8)
    np.testing.assert_array_equal(rows.view(np.int32), y1.view(np.int32))
    np.testing.assert_array_equal(lnq.astype(np.int64), ln[0])


def test_gelu_matches_oracle(layer):
    _, qp, _, vals = layer
    a, s_a, zpa = _q(layer, "/layernorm_after/LayerNormalization_output_0")
    bt, s_w = _w(layer, "onnx::MatMul_129")
    want, s_o, zp_o = _q(layer, "/intermediate/intermediate_act_fn/Mul_1_output_0")
    c = [vals[f"/intermediate/intermediate_act_fn/Constant{s}_output_0"][1] for s in ("", "_1", "_2")]
    assert np.float32(c[0]) == R.SQRT2_F32 and float(c[1]) == 1.0 and float(c[2]) == 0.5
    got = R.gelu(_i8(a[0]), bt, _bias(layer, "intermediate.dense.bias"), int(zpa), s_a * s_w, s_o, int(zp_o), 8,
                 float(c[0]), float(c[1]), float(c[2]))
    np.testing.assert_array_equal(got, want[0])
