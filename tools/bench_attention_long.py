#!/usr/bin/env python
"""Same-box A/B of the long-sequence attention (nqk_attention_long) against the three-launch
chain it replaces (NQK_ATTN_LONG=0: V transpose, scores GEMM, softmax + quantize, P V GEMM).

Kernel level: a ViT-Base encoder layer at T tokens (onnx_proto.retoken), calibrated, one forward
through the plan; then the layer's own Q / K / V (still in the workspace) and quantization
parameters go through both routes, alternating, HIP events around each route's launches.
Model level: the ViT-Base classifier at 384 px (577 tokens), one hipGraph per route, replayed
alternating; device.POOL's peak live bytes of each route's capture are the memory figures.
Writes profiles/attention_long.json."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-quant_amd"))
from numpy_quant import _lib, onnx_proto  # noqa: E402
from numpy_quant.device import POOL, DeviceArray, sync  # noqa: E402
from numpy_quant.model import Model  # noqa: E402
from numpy_quant.plan import FusedLayer, _f32, _zp  # noqa: E402

MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")


def stats(ts):
    ts = sorted(ts)
    return {"min": round(ts[0], 2), "median": round(ts[len(ts) // 2], 2), "max": round(ts[-1], 2), "n": len(ts)}


def events():
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.call("nqk_event_create", ctypes.byref(e0))
    _lib.call("nqk_event_create", ctypes.byref(e1))
    return e0, e1


def timed(fn, launches, ev):
    """Microseconds per call of fn, HIP events around `launches` calls."""
    fn()
    _lib.call("nqk_event_record", ev[0])
    for _ in range(launches):
        fn()
    _lib.call("nqk_event_record", ev[1])
    sync()
    ms = ctypes.c_float()
    _lib.call("nqk_event_elapsed", ev[0], ev[1], ctypes.byref(ms))
    return 1e3 * ms.value / launches


def kernel_ab(T, B, reps, launches):
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_encoder_layer_no_weights.onnx"),
                            synthetic_weights=True)
    onnx_proto.retoken(proto, T)
    model = Model.from_onnx(proto)
    model.rebatch(2)
    rng = np.random.default_rng(T)
    qmodel = model.quantize([rng.standard_normal((2, T, 768)).astype(np.float32)], bit_width=8)
    model.rebatch(B)
    os.environ["NQK_ATTN_LONG"] = "1"
    plan = qmodel.compile()
    qmodel([rng.standard_normal((B, T, 768)).astype(np.float32)])
    layer = [o for _, o in plan.steps if isinstance(o, FusedLayer)][0]
    assert layer.attn_long
    m = layer.m
    H, Dh, D = m.heads, m.hdim, layer.D
    Tp = (T + 15) // 16 * 16
    w = dict(plan.ws.bufs)
    pq, pk, pv_ = layer.p_head["q"], layer.p_head["k"], layer.p_head["v"]
    a = _lib.Attention()
    a.heads, a.tokens, a.hdim, a.ld_out, a.bit_width = H, T, Dh, D, layer.bw
    a.zq, a.zk = _zp(pq), _zp(pk)
    a.s_qk, a.div = _f32(np.float32(pq.scale) * np.float32(pk.scale)), m.div
    a.s_p, a.zp_p = _f32(layer.p_sm.scale), _zp(layer.p_sm)
    a.s_pv, a.zv = _f32(np.float32(layer.p_sm.scale) * np.float32(pv_.scale)), _zp(pv_)
    a.s_ctx, a.zp_ctx = _f32(layer.p_ctx.scale), _zp(layer.p_ctx)
    ctx_l = DeviceArray((B * T, D), np.int8)
    wc = {"q": w["q"], "k": w["k"], "v": w["v"], "ctx": DeviceArray((B * T, D), np.int8),
          "vt": DeviceArray((B * H, Dh, Tp), np.int8), "s": DeviceArray((B * H, T, T), np.float32),
          "p": DeviceArray((B * H, T, Tp), np.int8)}

    def long_():
        _lib.call("nqk_attention_long", w["q"].vp, w["k"].vp, w["v"].vp, ctx_l.vp, B * H, ctypes.byref(a))

    def chain():
        layer._attention_unfused(wc, B, T, Tp, H, Dh, D)

    ev = events()
    res = {"long": [], "chain": []}
    for _ in range(reps):
        res["long"].append(timed(long_, launches, ev))
        res["chain"].append(timed(chain, launches, ev))
    equal = bool(np.array_equal(ctx_l.to_host(), wc["ctx"].to_host()))
    out = {"tokens": T, "batch": B, "heads": H, "params": {"zq": a.zq, "zk": a.zk, "zp_p": a.zp_p, "zv": a.zv, "s_p": a.s_p},
           "long_us": stats(res["long"]), "chain_us": stats(res["chain"]), "bit_identical": equal,
           "chain_workspace_bytes": sum(wc[k].nbytes for k in ("vt", "s", "p"))}
    print(json.dumps(out), flush=True)
    return out


def model_ab(B, reps, launches):
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
    onnx_proto.retoken(proto, image=384)
    model = Model.from_onnx(proto)
    model.rebatch(2)
    rng = np.random.default_rng(384)
    qmodel = model.quantize([rng.standard_normal((2, 3, 384, 384)).astype(np.float32)], bit_width=8)
    for v in model.values:  # free the float calibration activations
        if v.__class__.__name__ == "Variable":
            v.data = None
    model.rebatch(B)
    x = rng.standard_normal((B, 3, 384, 384)).astype(np.float32)
    graphs, peak, outs = {}, {}, {}
    for leg in ("1", "0"):
        os.environ["NQK_ATTN_LONG"] = leg
        qmodel._plan = None
        POOL.trim()
        base = POOL.live_bytes
        POOL.peak_bytes = base
        g = qmodel.graph([x])
        layers = [o for k, o in g.plan.steps if k == "layer"]
        assert all(l.attn_long == (leg == "1") for l in layers) and len(layers) == 12
        outs[leg] = g([x])[0]
        peak[leg] = POOL.peak_bytes
        graphs[leg] = g
    from numpy_quant.tensor import FTensor
    xd = FTensor(x)
    ev = events()
    res = {"1": [], "0": []}
    for _ in range(reps):
        for leg in ("1", "0"):
            res[leg].append(timed(lambda: graphs[leg].run_device([xd]), launches, ev) / 1e3)
    for g in graphs.values():
        g.destroy()
    out = {"model": "ViT-Base/16 classifier, 384 px, 577 tokens, int8", "batch": B,
           "long_ms": stats(res["1"]), "chain_ms": stats(res["0"]),
           "bit_identical": bool(np.array_equal(outs["1"], outs["0"])),
           "pool_peak_live_bytes": {"long": peak["1"], "chain": peak["0"]}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--model-batch", type=int, default=64)
    ap.add_argument("--model-launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_long.json"))
    args = ap.parse_args()
    _lib.ensure_init(0)
    result = {"tool": "tools/bench_attention_long.py", "unit": "min / median / max over --reps alternating repetitions",
              "kernel": [kernel_ab(577, 64, args.reps, args.launches), kernel_ab(1025, 16, args.reps, args.launches)],
              "model": model_ab(args.model_batch, args.reps, args.model_launches)}
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
