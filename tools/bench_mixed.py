#!/usr/bin/env python
"""A separate weight bit width (QModel.weight_bit_width): 4-bit weights under 8-bit activations
against the two models that existed before it, (8, 8) and (4, 4), on one MI355X.  Prints one JSON
line (and writes it to --out, e.g. profiles/mixed_width.json).

  error   the encoder-layer graph with seeded stand-in weights whose columns are spread
          log-uniformly over 2^-3..2^3 (the tests' accuracy fixture), batch 2: model.compare's
          output MSE and SQNR at (activation, weight) widths (8, 8), (8, 4) and (4, 4), per tensor
          and per column
  step    the graph-replayed ViT-Base forward (synthetic weights, B = 256) of the same three models,
          and (8, 4) once more captured under NQK_PG_NOS8=1: the nibble QKV instance with the
          saturating 8-bit store against the clamped one it replaces.  Every replay is checked
          against its plain call, and every projection GEMM's kernel id is asserted (k_pg)

The legs of a step alternate in one process; a figure is the median of its --rounds windows,
with min-max.  Each GPU step is a child process under its own time limit; after a step that
fails or runs out of time nothing more is started.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "numpy-quant_amd"), ROOT):
    sys.path.insert(0, p)

MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
WIDTHS = ((8, 8), (8, 4), (4, 4))  # (activation, weight)


def _timer_ms(fn) -> float:
    from numpy_quant import _lib
    _lib.call("nqk_timer_start")
    fn()
    _lib.call("nqk_timer_stop")
    ms = ctypes.c_float()
    _lib.call("nqk_timer_ms", ctypes.byref(ms))
    return ms.value


def _stats(samples, digits=3):
    return round(statistics.median(samples), digits), [round(min(samples), digits), round(max(samples), digits)]


def step_error(args) -> dict:
    from numpy_quant.model import Model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _perchannel_ref as R
    proto, _, x = R.encoder_layer_fixture(MODELS, seed=R.SEED, batch=2)
    model = Model.from_onnx(proto)
    out = model.outputs[0].name
    res = {"error_rows": int(x.shape[0] * x.shape[1])}
    for bw, wbw in WIDTHS:
        for tag, pc in (("per_tensor", False), ("per_channel", True)):
            q = model.quantize([x], bit_width=bw, weight_bit_width=wbw, per_channel=pc)
            s = model.compare(q, [[x]], k=1).values[out]
            res[f"error_a{bw}w{wbw}_{tag}_output_mse"] = float(s.mse)
            res[f"error_a{bw}w{wbw}_{tag}_output_sqnr_db"] = round(float(s.sqnr_db), 3)
    return res


def _forward_kernels(q, x_dev):
    """One plain forward; returns (logits, {kernel id: launches}) of its projection GEMMs."""
    from numpy_quant import _lib, plan
    ids = {}
    real = plan._gemm

    def spy(epi, *rest):
        real(epi, *rest)
        if epi in (plan.EPI_QKV, plan.EPI_RESID, plan.EPI_GELU):
            k = int(_lib.load().nqk_qgemm_last_kernel())
            ids[k] = ids.get(k, 0) + 1

    plan._gemm = spy
    try:
        logits = q([x_dev])[0]
    finally:
        plan._gemm = real
    return logits, ids


def step_step(args) -> dict:
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    from numpy_quant.tensor import FTensor
    B = args.step_batch
    x_cal = np.random.default_rng(12345).standard_normal((8, 3, 224, 224)).astype(np.float32)
    x_dev = FTensor(np.random.default_rng(256).standard_normal((B, 3, 224, 224)).astype(np.float32))
    model = Model.from_onnx(onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"),
                                            synthetic_weights=True))
    model.rebatch(8)
    legs = [(f"a{bw}w{wbw}", bw, wbw, False) for bw, wbw in WIDTHS] + [("a8w4_nos8", 8, 4, True)]
    qs = {name: model.quantize([x_cal], bit_width=bw, weight_bit_width=wbw) for name, bw, wbw, _ in legs}
    for v in model.values:  # free the float calibration activations
        if v.__class__.__name__ == "Variable":
            v.data = None
    model.rebatch(B)
    res = {"step_batch": B}
    graphs, logits = {}, {}
    for name, bw, wbw, nos8 in legs:
        q = qs[name]
        # the launcher reads NQK_PG_NOS8 at every launch: the plain call and the capture both run under it
        if nos8:
            os.environ["NQK_PG_NOS8"] = "1"
        try:
            logits[name], ids = _forward_kernels(q, x_dev)
            if not ids or set(ids) - {4, 5, 6, 7}:
                raise AssertionError(f"{name}: projection GEMMs off k_pg: kernel ids {ids}")
            res[f"{name}_gemm_kernel_ids"] = {str(k): n for k, n in sorted(ids.items())}
            res[f"{name}_fused_layers"] = q._plan.fused
            graphs[name] = q.graph([x_dev])
            if not np.array_equal(graphs[name].run_device([x_dev])[0].dev.to_host(), logits[name]):
                raise AssertionError(f"graph replay differs from the plain call ({name})")
        finally:
            os.environ.pop("NQK_PG_NOS8", None)
    if not np.array_equal(logits["a8w4"], logits["a8w4_nos8"]):
        raise AssertionError("the saturating-store QKV instance and the clamped one give different logits")
    samples = {k: [] for k in graphs}
    for i in range(args.warmup + args.rounds):
        for name, g in graphs.items():
            ms = _timer_ms(lambda: [g.run_device([x_dev]) for _ in range(args.steps)])
            if i >= args.warmup:
                samples[name].append(ms / args.steps)
    for name, smp in samples.items():
        res[f"step_{name}_ms"], res[f"step_{name}_ms_min_max"] = _stats(smp)
        res[f"step_{name}_images_per_s"] = round(1e3 * B / res[f"step_{name}_ms"], 1)
    for a, b in (("a8w4", "a8w8"), ("a4w4", "a8w8"), ("a8w4", "a4w4")):
        res[f"top1_agreement_{a}_vs_{b}"] = float(np.mean(logits[a].argmax(1) == logits[b].argmax(1)))
    for g in graphs.values():
        g.destroy()
    return res


STEPS = {"error": (step_error, 240), "step": (step_step, 540)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step-batch", type=int, default=256, help="images of the graph-replayed forward")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5, help="graph replays per timed window")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "4-bit weights under 8-bit activations (QModel.weight_bit_width) against (8, 8) and (4, 4)",
              "rounds": args.rounds}
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("step_batch", "rounds", "warmup", "steps")]
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_mixed] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_mixed] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
            return p.returncode or 1
        result.update(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
