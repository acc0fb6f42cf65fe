#!/usr/bin/env python
"""Per-column weight scales (QModel.per_channel) against the reference's one scale per weight, on
one MI355X.  Prints one JSON line (and writes it to --out, e.g. profiles/per_channel.json).

  error   the encoder-layer graph with seeded stand-in weights whose columns are spread
          log-uniformly over 2^-3..2^3 (the tests' accuracy fixture), batch 2: model.compare's
          output MSE and SQNR at 4 and 8 bits, per tensor and per column, and the weights' own SQNR
  kernel  nqk_dequantize_cols / nqk_requantize_cols against their scalar twins on an int32
          [rows, 768] accumulator, library stream timer: us per launch
  step    the graph-replayed ViT-Base forward (synthetic weights, B = 256) at 8 and at 4 bits, per
          tensor and per column (nqk_epilogue.s_col: k_pg's per-column variant),
          and the four projection GEMMs' kernel times of a plain forward of each

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


def _spread_layer(batch=2):
    """The tests' accuracy fixture itself (tests/_perchannel_ref.encoder_layer_fixture): every MatMul
    weight's columns times 2^u, u uniform in [-3, 3], and its seeded input batch."""
    from numpy_quant.model import Model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _perchannel_ref as R
    proto, _, x = R.encoder_layer_fixture(MODELS, seed=R.SEED, batch=batch)
    return Model.from_onnx(proto), x


def step_error(args) -> dict:
    from numpy_quant.model import per_channel_axis
    model, x = _spread_layer()
    out = model.outputs[0].name
    weights = [v.name for v in model.values if per_channel_axis(v) is not None]
    res = {"error_rows": int(x.shape[0] * x.shape[1]), "error_weights": len(weights)}
    for bw in (4, 8):
        for tag, pc in (("per_tensor", False), ("per_channel", True)):
            q = model.quantize([x], bit_width=bw, per_channel=pc)
            rep = model.compare(q, [[x]], k=1)
            s = rep.values[out]
            res[f"error_bw{bw}_{tag}_output_mse"] = float(s.mse)
            res[f"error_bw{bw}_{tag}_output_sqnr_db"] = round(float(s.sqnr_db), 3)
            sq = [rep.values[w].sqnr_db for w in weights]
            res[f"error_bw{bw}_{tag}_weight_sqnr_db_min_max"] = [round(min(sq), 2), round(max(sq), 2)]
    return res


def step_kernel(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray, sync
    rng = np.random.default_rng(0)
    rows, n = args.batch * 197, 768
    acc = DeviceArray.from_host(rng.integers(-200000, 200000, size=(rows, n)).astype(np.int32))
    s = (np.float32(1e-4) * np.exp2(rng.uniform(-3, 3, size=n))).astype(np.float32)
    sdev = DeviceArray.from_host(s)
    legs = {"dequantize": lambda: K.dequantize(acc, s[0], None),
            "dequantize_cols": lambda: K.dequantize_cols(acc, sdev, None),
            "requantize": lambda: K.requantize(acc, s[0], None, None, np.float32(0.2), -3, 8),
            "requantize_cols": lambda: K.requantize_cols(acc, sdev, None, None, np.float32(0.2), -3, 8)}
    samples = {k: [] for k in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            ms = _timer_ms(lambda: [fn() for _ in range(args.reps)])
            if i >= args.warmup:
                samples[name].append(1e3 * ms / args.reps)
    sync()
    res = {"kernel_rows": rows, "kernel_cols": n}
    for name, smp in samples.items():
        res[f"{name}_us"], res[f"{name}_us_min_max"] = _stats(smp, 2)
    return res


def step_step(args) -> dict:
    """Per bit width (8, 4): both models' graph-replayed step, alternating, and the four projection
    GEMMs' kernel times of one plain forward each (kernels.KernelTimer: the median over the layers)."""
    from numpy_quant import kernels as K
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    from numpy_quant.tensor import FTensor
    B = args.step_batch
    x_cal = np.random.default_rng(12345).standard_normal((8, 3, 224, 224)).astype(np.float32)
    x_dev = FTensor(np.random.default_rng(256).standard_normal((B, 3, 224, 224)).astype(np.float32))
    res = {"step_batch": B}
    for bw in (8, 4):
        model = Model.from_onnx(onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"),
                                                synthetic_weights=True))
        model.rebatch(8)
        qs = {"per_tensor": model.quantize([x_cal], bit_width=bw),
              "per_channel": model.quantize([x_cal], bit_width=bw, per_channel=True)}
        for v in model.values:  # free the float calibration activations
            if v.__class__.__name__ == "Variable":
                v.data = None
        model.rebatch(B)
        graphs, logits = {}, {}
        for name, q in qs.items():
            logits[name] = q([x_dev])[0]
            K.TIMER = K.KernelTimer()
            try:
                q([x_dev])
                recs = K.TIMER.collect()
            finally:
                K.TIMER = None
            for tag in ("qgemm_qkv", "qgemm_out", "qgemm_gelu", "qgemm_down"):
                # per launch (a half batch per stream where the plan splits); layers without the CLS tail
                us = sorted(1e3 * ms for t, ms, _, _ in recs if t == tag)
                res[f"bw{bw}_{name}_{tag}_us"] = round(statistics.median(us), 1)
                res[f"bw{bw}_{name}_{tag}_us_min_max"] = [round(us[0], 1), round(us[-1], 1)]
                res[f"bw{bw}_{name}_{tag}_launches"] = len(us)
            graphs[name] = q.graph([x_dev])
            if not np.array_equal(graphs[name].run_device([x_dev])[0].dev.to_host(), logits[name]):
                raise AssertionError(f"graph replay differs from the plain call ({name}, {bw} bits)")
        samples = {k: [] for k in graphs}
        for i in range(args.warmup + args.rounds):
            for name, g in graphs.items():
                ms = _timer_ms(lambda: [g.run_device([x_dev]) for _ in range(args.steps)])
                if i >= args.warmup:
                    samples[name].append(ms / args.steps)
        res[f"bw{bw}_fused_layers"] = {k: q._plan.fused for k, q in qs.items()}
        for name, smp in samples.items():
            res[f"bw{bw}_step_{name}_ms"], res[f"bw{bw}_step_{name}_ms_min_max"] = _stats(smp)
        res[f"bw{bw}_top1_agreement_per_channel_vs_per_tensor"] = float(
            np.mean(logits["per_channel"].argmax(1) == logits["per_tensor"].argmax(1)))
        for g in graphs.values():
            g.destroy()
        del graphs, qs, model
    return res


STEPS = {"error": (step_error, 240), "kernel": (step_kernel, 120), "step": (step_step, 540)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256, help="images of the kernel step's accumulator")
    ap.add_argument("--step-batch", type=int, default=256, help="images of the graph-replayed forward")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="kernel launches per timed window")
    ap.add_argument("--steps", type=int, default=5, help="graph replays per timed window")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "per-column weight scales (QModel.per_channel) against one scale per weight",
              "rounds": args.rounds}
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}"
                   for k in ("batch", "step_batch", "rounds", "warmup", "reps", "steps")]
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_perchannel] step {name} ran past its {limit} s limit; nothing more is started",
                  file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_perchannel] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
