"""The fused plan on graphs past 224 tokens (onnx_proto.retoken): the layer takes the long-sequence
one-kernel attention (plan.FusedLayer.attn_long, nqk_attention_long), keeps the two-stream parts
and the CLS tail, allocates no score / probability workspace, and computes the node loop's bits;
NQK_ATTN_LONG=0 keeps the three launches with the same bits.  At batch 1 the node loop and both
plans are also compared with the oracle's quantized_forward."""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
IMAGENET = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
_CACHE = {}


def _layers(plan):
    return [s for k, s in plan.steps if k == "layer"]


def _layer_model(kw_key):
    """(qmodel, x, node-loop output) of the ViT-Ti encoder layer at 226 tokens, batch 3, built once
    per quantization setting."""
    if kw_key not in _CACHE:
        from numpy_quant import onnx_proto
        from numpy_quant.model import Model
        proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_encoder_layer_no_weights.onnx"),
                                synthetic_weights=True)
        assert onnx_proto.redimension(proto, 192, 3, 768) > 0
        assert onnx_proto.retoken(proto, 226) == 6  # 4 shape constants, the input, the output
        onnx_proto.rebatch(proto, 3)
        x = np.random.default_rng(226).standard_normal((3, 226, 192)).astype(np.float32)
        qmodel = Model.from_onnx(proto).quantize([x], **dict(kw_key))
        qmodel.keep_values = True
        eager = qmodel([x])[0]
        qmodel.keep_values = False
        assert eager.shape == (3, 226, 192)
        _CACHE[kw_key] = (qmodel, x, eager)
    return _CACHE[kw_key]


QUANT = {"int8": (("bit_width", 8),), "int4": (("bit_width", 4),),
         "per_channel_w4": (("bit_width", 8), ("per_channel", True), ("weight_bit_width", 4))}


@pytest.mark.parametrize("quant", sorted(QUANT))
def test_encoder_layer_226_tokens(quant, monkeypatch):
    qmodel, x, eager = _layer_model(QUANT[quant])
    monkeypatch.delenv("NQK_ATTN_LONG", raising=False)
    plan = qmodel.compile()
    (layer,) = _layers(plan)
    assert plan.fused == 1 and layer.attn_long and not layer.attn_fused
    assert plan.split
    np.testing.assert_array_equal(qmodel([x])[0], eager)      # two streams: images 2 + 1
    assert "s" not in plan.ws.bufs and "p" not in plan.ws.bufs and "vt" not in plan.ws.bufs
    plan.split = False
    np.testing.assert_array_equal(qmodel([x])[0], eager)      # one stream
    # the A/B leg: three launches, the same bits
    monkeypatch.setenv("NQK_ATTN_LONG", "0")
    plan = qmodel.compile()
    (layer,) = _layers(plan)
    assert plan.fused == 1 and not layer.attn_long and not layer.attn_fused
    np.testing.assert_array_equal(qmodel([x])[0], eager)
    assert "s" in plan.ws.bufs and "p" in plan.ws.bufs


def test_encoder_layer_226_tokens_matches_oracle(monkeypatch):
    """The same graph at batch 1 against the oracle's quantized_forward (as
    test_gpu_plan.test_plan_encoder_layer_graph_matches_oracle at 197 tokens): the node loop, the
    plan with nqk_attention_long and the plan with the three launches all compute the oracle's bits."""
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model, QuantizationParams
    from oracle import nq_oracle as O

    def proto():
        p = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_encoder_layer_no_weights.onnx"), synthetic_weights=True)
        assert onnx_proto.redimension(p, 192, 3, 768) > 0
        assert onnx_proto.retoken(p, 226) == 6
        return p

    x = np.random.default_rng(226).standard_normal((1, 226, 192)).astype(np.float32)
    graph = O.Graph(proto())
    with np.errstate(all="ignore"):
        qp, qc = O.calibrate(graph, [x], 8)
        ref = O.outputs_of(graph, O.quantized_forward(graph, qp, qc, [x], 8))[0]
    assert ref.shape == (1, 226, 192)
    qmodel = Model.from_onnx(proto()).quantize_with({k: QuantizationParams(v.scale, v.zero_point) for k, v in qp.items()},
                                                    bit_width=8)
    qmodel.keep_values = True
    np.testing.assert_array_equal(qmodel([x])[0], ref)
    qmodel.keep_values = False
    monkeypatch.delenv("NQK_ATTN_LONG", raising=False)
    (layer,) = _layers(qmodel.compile())
    assert layer.attn_long and not layer.attn_fused
    np.testing.assert_array_equal(qmodel([x])[0], ref)
    monkeypatch.setenv("NQK_ATTN_LONG", "0")
    (layer,) = _layers(qmodel.compile())
    assert not layer.attn_long and not layer.attn_fused
    np.testing.assert_array_equal(qmodel([x])[0], ref)


def test_fused_attention_switch_forces_three_launches(monkeypatch):
    from numpy_quant import plan as P
    qmodel, x, eager = _layer_model(QUANT["int8"])
    monkeypatch.delenv("NQK_ATTN_LONG", raising=False)
    monkeypatch.setattr(P, "FUSED_ATTENTION", False)
    (layer,) = _layers(qmodel.compile())
    assert not layer.attn_long and not layer.attn_fused
    np.testing.assert_array_equal(qmodel([x])[0], eager)


def test_plan_predicate_matches_the_entry_point():
    """plan.attn_long_accepts is nqk_attention_long's own host check."""
    from numpy_quant import _lib
    from numpy_quant.plan import attn_long_accepts
    ok = (1e-3, 8.0, 1 / 255, 1e-4, 0.02)
    assert attn_long_accepts(577, 64, 8, 4096, -4096, 1024, -1024, ok)
    assert attn_long_accepts(_lib.ATTN_LONG_MAX_T, 64, 8, 0, 0, -128, 3, ok)
    assert not attn_long_accepts(_lib.ATTN_LONG_MAX_T, 64, 8, 0, 0, 1024, -1024, ok)  # the int32 bound at this length
    assert not attn_long_accepts(224, 64, 8, 0, 0, -128, 3, ok)
    assert not attn_long_accepts(_lib.ATTN_LONG_MAX_T + 1, 64, 8, 0, 0, -128, 3, ok)
    assert not attn_long_accepts(577, 32, 8, 0, 0, -128, 3, ok)
    assert not attn_long_accepts(577, 64, 8, 0, 0, -128, 3, (1e-3, 8.0, 1e-40, 1e-4, 0.02))


def _classifier():
    """(qmodel, x, node-loop logits) of the ViT-Ti classifier at 240 px (226 tokens), batch 2."""
    if "cls" not in _CACHE:
        from numpy_quant import onnx_proto
        from numpy_quant.model import Model
        proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
        assert onnx_proto.redimension(proto, 192, 3, 768) > 0
        assert onnx_proto.retoken(proto, image=240) == 36 + 12 + 1 + 1  # shape constants, position embeddings, input
        onnx_proto.rebatch(proto, 2)
        x = np.random.default_rng(240).standard_normal((2, 3, 240, 240)).astype(np.float32)
        qmodel = Model.from_onnx(proto).quantize([x], bit_width=8)
        qmodel.keep_values = True
        eager = qmodel([x])[0]
        qmodel.keep_values = False
        assert eager.shape == (2, 1000)
        _CACHE["cls"] = (qmodel, x, eager)
    return _CACHE["cls"]


def test_classifier_240px_cls_tail_and_graph_replay(monkeypatch):
    from numpy_quant.plan import FusedAway
    monkeypatch.delenv("NQK_ATTN_LONG", raising=False)
    monkeypatch.delenv("NQK_NO_CLS_TAIL", raising=False)
    qmodel, x, eager = _classifier()
    plan = qmodel.compile()
    layers = _layers(plan)
    assert plan.fused == 12 and all(l.attn_long for l in layers)
    assert [l.cls_tail for l in layers] == [False] * 11 + [True]   # nqk_attention_long with q_rows = 1
    out = qmodel([x])[0]
    np.testing.assert_array_equal(out, eager)
    assert "s" not in plan.ws.bufs and "p" not in plan.ws.bufs
    idx, prob = qmodel.classify([x], 5)
    np.testing.assert_array_equal(idx, np.argsort(-eager, axis=1, kind="stable")[:, :5])
    x2 = np.random.default_rng(241).standard_normal(x.shape).astype(np.float32)
    want2 = qmodel([x2])[0]
    g = qmodel.graph([x])
    try:
        last = _layers(g.plan)[-1]
        assert last.cls_tail and last.attn_long and isinstance(last.m.x_out.data, FusedAway)
        np.testing.assert_array_equal(g([x2])[0], want2)
        np.testing.assert_array_equal(g([x])[0], eager)
    finally:
        g.destroy()


def test_classifier_240px_classify_stream(monkeypatch):
    """uint8 images through classify_stream equal the float path of the same pixels."""
    from numpy_quant.images import ImagePreprocess
    monkeypatch.delenv("NQK_ATTN_LONG", raising=False)
    qmodel, x, eager = _classifier()
    pre = ImagePreprocess(*IMAGENET)
    rng = np.random.default_rng(7)
    batches = [rng.integers(0, 256, size=(2, 240, 240, 3), dtype=np.uint8) for _ in range(2)]
    old = qmodel.image_preprocess
    qmodel.image_preprocess = pre
    try:
        assert all(l.attn_long for l in _layers(qmodel.compile()))
        want = [qmodel([b])[0] for b in batches]
        got = list(qmodel.classify_stream(iter(batches)))
    finally:
        qmodel.image_preprocess = old
    assert len(got) == 2 and not np.array_equal(want[0], want[1])
    for g_, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g_), np.asarray(w))
