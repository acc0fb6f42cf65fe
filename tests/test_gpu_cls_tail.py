"""The CLS tail of the fused plan (plan.FusedLayer.cls_tail): the last encoder layer of a CLS-pooled
ViT computes, after K and V, only the token-0 rows the classifier reads.  The logits equal the
unpruned plan's (NQK_NO_CLS_TAIL=1) and the node loop's bit for bit; the layer's full output is
still there for a reader (plan.DeferredRows)."""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")

# config: (ViT-Ti dimensions?, batch, bit width); batch 3 gives uneven halves (2 + 1 images)
CONFIGS = {"base_b3_int8": (False, 3, 8), "base_b2_int4": (False, 2, 4), "tiny_b3_int8": (True, 3, 8)}
_CACHE = {}


def _config(name):
    """(qmodel, x, node-loop logits) of a config, built once."""
    if name not in _CACHE:
        from numpy_quant import onnx_proto
        from numpy_quant.model import Model
        tiny, batch, bw = CONFIGS[name]
        proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
        if tiny:
            assert onnx_proto.redimension(proto, 192, 3, 768) > 0
        onnx_proto.rebatch(proto, batch)
        x = np.random.default_rng(40 + batch + bw).standard_normal((batch, 3, 224, 224)).astype(np.float32)
        qmodel = Model.from_onnx(proto).quantize([x], bit_width=bw)
        qmodel.keep_values = True
        eager = qmodel([x])[0]
        qmodel.keep_values = False
        _CACHE[name] = (qmodel, x, eager)
    return _CACHE[name]


def _layers(plan):
    return [s for k, s in plan.steps if k == "layer"]


def _compile(qmodel, monkeypatch, tail):
    if tail:
        monkeypatch.delenv("NQK_NO_CLS_TAIL", raising=False)
    else:
        monkeypatch.setenv("NQK_NO_CLS_TAIL", "1")
    return qmodel.compile()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_logits_equal_unpruned_plan_and_node_loop(name, monkeypatch):
    qmodel, x, eager = _config(name)
    plan = _compile(qmodel, monkeypatch, True)
    assert plan.fused == 12 and plan.pushdowns == 1
    assert [l.cls_tail for l in _layers(plan)] == [False] * 11 + [True]
    pruned = qmodel([x])[0]
    full_plan = _compile(qmodel, monkeypatch, False)
    assert not any(l.cls_tail for l in _layers(full_plan))
    unpruned = qmodel([x])[0]
    np.testing.assert_array_equal(pruned, unpruned)
    np.testing.assert_array_equal(pruned, eager)


def test_one_stream(monkeypatch):
    qmodel, x, eager = _config("base_b3_int8")
    plan = _compile(qmodel, monkeypatch, True)
    plan.split = False
    np.testing.assert_array_equal(qmodel([x])[0], eager)


def test_no_tail_without_fused_attention(monkeypatch):
    from numpy_quant import plan as P
    qmodel, _, _ = _config("base_b2_int4")
    monkeypatch.setattr(P, "FUSED_ATTENTION", False)
    plan = _compile(qmodel, monkeypatch, True)
    assert plan.fused == 12 and not any(l.cls_tail for l in _layers(plan))


def test_no_tail_when_the_layer_output_is_a_graph_output(monkeypatch):
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    path = os.path.join(MODELS, "vit_image_classifier_encoder_layer_no_weights.onnx")
    x = np.random.default_rng(5).standard_normal((1, 197, 768)).astype(np.float32)
    qmodel = Model.from_onnx(onnx_proto.load(path, synthetic_weights=True)).quantize([x], bit_width=8)
    plan = _compile(qmodel, monkeypatch, True)
    assert plan.fused == 1 and not any(l.cls_tail for l in _layers(plan))


def test_deferred_layer_output(monkeypatch):
    """Reading the pruned layer's output value computes every row: the unpruned plan's tensor, byte
    for byte; the logits of that run and of the next are unchanged; a value not read before the next
    run raises instead of reading a reused workspace."""
    from numpy_quant.plan import DeferredRows, FusedAwayError
    qmodel, x, eager = _config("base_b3_int8")
    plan = _compile(qmodel, monkeypatch, True)
    last = _layers(plan)[-1]
    np.testing.assert_array_equal(qmodel([x])[0], eager)
    unread = last.m.x_out.data
    assert isinstance(unread, DeferredRows)
    np.testing.assert_array_equal(qmodel([x])[0], eager)
    with pytest.raises(FusedAwayError):
        unread.data
    value = last.m.x_out.data
    assert value is not unread and tuple(value.shape.data) == (3, 197, 768)
    rows = np.array(value.data)
    np.testing.assert_array_equal(qmodel.outputs_device()[0].dev.to_host(), eager)
    np.testing.assert_array_equal(qmodel([x])[0], eager)
    np.testing.assert_array_equal(value.data, rows)  # materialised: the next run leaves it alone
    full_plan = _compile(qmodel, monkeypatch, False)
    np.testing.assert_array_equal(qmodel([x])[0], eager)
    want = _layers(full_plan)[-1].m.x_out.data.data
    assert rows.dtype == want.dtype and rows.tobytes() == want.tobytes()


def test_graph_replay(monkeypatch):
    from numpy_quant.plan import FusedAway
    qmodel, x, _ = _config("base_b2_int4")
    _compile(qmodel, monkeypatch, True)
    xs = [x, np.random.default_rng(77).standard_normal(x.shape).astype(np.float32)]
    want = [qmodel([a])[0] for a in xs]
    g = qmodel.graph([xs[0]])
    try:
        last = _layers(g.plan)[-1]
        assert last.cls_tail and isinstance(last.m.x_out.data, FusedAway)
        np.testing.assert_array_equal(g([xs[1]])[0], want[1])
        np.testing.assert_array_equal(g([xs[0]])[0], want[0])
    finally:
        g.destroy()
