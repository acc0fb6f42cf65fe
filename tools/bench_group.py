#!/usr/bin/env python
"""nqk_qgemm_group (group-wise weight scales, the rescale inside the k loop) on one MI355X.  Prints
one JSON line (and writes it to --out, e.g. profiles/group_scales.json).

  gemm    ViT-Base's four projection shapes at --gemm-batch images, g = 32, 64 and 128:
          kernels.qmatmul_group beside the nearest existing route on the same operands,
          nqk_qgemm_i8 followed by nqk_dequantize_cols (which computes the per-column result, not
          the same one).  The kernel alone (KernelTimer, "qgemm_group") gives the share of the int8
          MFMA peak and the bytes per second
  model   the node-loop forward of ViT-Base (synthetic weights) at (8, 4) with group_size=128
          against (8, 4) per_channel=True, at --model-batch and --model-batch-large images
  error   model.compare's output MSE and SQNR on the two encoder-layer fixtures of
          tools/bench_weight_clip.py at (8, 4) and (4, 4): per tensor, per column, g = 32, 64, 128

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
INT8_PEAK_OPS = 256 * 2.4e9 * 8192  # bench.py INT8_PEAK_TOPS: dense int8 MFMA operations per second
T, D = 197, 768
SHAPES = {"qkv": (D, 3 * D), "out_proj": (D, D), "ffn_up": (D, 4 * D), "ffn_down": (4 * D, D)}  # name: (K, N)
GROUPS = (32, 64, 128)


def _timer_ms(fn) -> float:
    from numpy_quant import _lib
    _lib.call("nqk_timer_start")
    fn()
    _lib.call("nqk_timer_stop")
    ms = ctypes.c_float()
    _lib.call("nqk_timer_ms", ctypes.byref(ms))
    return ms.value


def _stats(samples, digits=4):
    return round(statistics.median(samples), digits), [round(min(samples), digits), round(max(samples), digits)]


def step_gemm(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rng = np.random.default_rng(16)
    M = args.gemm_batch * T
    res = {"gemm_batch": args.gemm_batch, "gemm_M": M}
    for name, (Kd, N) in SHAPES.items():
        a = DeviceArray.from_host(rng.integers(-128, 128, size=(M, Kd), dtype=np.int8))
        b = DeviceArray.from_host(rng.integers(-8, 8, size=(Kd, N)).astype(np.int8))
        bt, col = K.weight_bt(b)
        scol = DeviceArray.from_host(np.exp2(rng.uniform(-12, -8, size=N)).astype(np.float32))

        def per_column():
            acc, zt = K.qmatmul(a, b, 3, None, bt, col)
            return K.dequantize_cols(acc, scol, zt)
        for g in GROUPS:
            sg = DeviceArray.from_host(np.exp2(rng.uniform(-12, -8, size=(Kd // g, N))).astype(np.float32))
            gsum = K.group_colsum(bt, g)
            legs = {"group": lambda: K.qmatmul_group(a, bt, gsum, sg, 3, g), "i8_dequant": per_column}
            samples = {leg: [] for leg in legs}
            for i in range(args.warmup + args.rounds):
                for leg, call in legs.items():
                    ms = _timer_ms(lambda: [call() for _ in range(args.reps)]) / args.reps
                    if i >= args.warmup:
                        samples[leg].append(ms)
            key = f"gemm_{name}_g{g}"
            for leg in legs:
                res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = _stats(samples[leg])
            res[f"{key}_ratio_to_i8_dequant"] = round(res[f"{key}_group_ms"] / res[f"{key}_i8_dequant_ms"], 3)
            K.TIMER = K.KernelTimer()  # the kernel alone
            for _ in range(args.rounds):
                legs["group"]()
            legs["group"]().to_host()  # a synchronising call: every event has passed
            recs = [r for r in K.TIMER.collect() if r[0] == "qgemm_group"]
            K.TIMER = None
            ms = statistics.median(r[1] for r in recs)
            res[f"{key}_kernel_ms"] = round(ms, 4)
            res[f"{key}_mfma_peak_share"] = round(recs[0][2][0] / (ms * 1e-3) / INT8_PEAK_OPS, 4)
            res[f"{key}_kernel_tb_per_s"] = round(recs[0][2][1] / (ms * 1e-3) / 1e12, 3)
    return res


def step_model(args) -> dict:
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    res = {"model_batches": [args.model_batch, args.model_batch_large]}
    for B in res["model_batches"]:
        x = np.random.default_rng(12345).standard_normal((B, 3, 224, 224)).astype(np.float32)
        proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
        onnx_proto.rebatch(proto, B)
        model = Model.from_onnx(proto)
        qs = {"group128": model.quantize([x], bit_width=8, weight_bit_width=4, group_size=128),
              "per_column": model.quantize([x], bit_width=8, weight_bit_width=4, per_channel=True)}
        for q in qs.values():
            q.keep_values = True  # the node loop on both legs
        samples = {leg: [] for leg in qs}
        for i in range(args.warmup + args.rounds):
            for leg, q in qs.items():
                ms = _timer_ms(lambda: q([x]))
                if i >= args.warmup:
                    samples[leg].append(ms)
        key = f"model_b{B}_a8w4"
        for leg in qs:
            res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = _stats(samples[leg], 2)
        res[f"{key}_ratio"] = round(res[f"{key}_group128_ms"] / res[f"{key}_per_column_ms"], 3)
        res[f"{key}_ranges_overlap"] = bool(max(samples["group128"]) >= min(samples["per_column"]) and
                                            max(samples["per_column"]) >= min(samples["group128"]))
        del qs
    return res


def step_error(args) -> dict:
    from numpy_quant.model import Model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _equalize_ref as E
    import _perchannel_ref as P
    proto, _, xs = P.encoder_layer_fixture(MODELS)
    oproto, _, xo, _ = E.outlier_fixture(MODELS)
    fixtures = {"spread_columns": (Model.from_onnx(proto), xs),
                "equalized_outliers": (Model.from_onnx(oproto).equalize([[xo]]), xo)}
    cells = [("per_tensor", {}), ("per_column", {"per_channel": True})] + [(f"g{g}", {"group_size": g}) for g in GROUPS]
    res = {}
    for fixture, (model, x) in fixtures.items():
        out = model.outputs[0].name
        for bw in (8, 4):
            for cell, kw in cells:
                q = model.quantize([x], bit_width=bw, weight_bit_width=4, **kw)
                s = model.compare(q, [[x]], k=1).values[out]
                res[f"error_{fixture}_a{bw}w4_{cell}_mse"] = float(s.mse)
                res[f"error_{fixture}_a{bw}w4_{cell}_sqnr_db"] = round(float(s.sqnr_db), 3)
    return res


STEPS = {"gemm": (step_gemm, 300), "model": (step_model, 600), "error": (step_error, 300)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gemm-batch", type=int, default=64, help="images behind the GEMM shapes")
    ap.add_argument("--model-batch", type=int, default=8, help="images of the node-loop forward")
    ap.add_argument("--model-batch-large", type=int, default=64, help="the second batch of the forward")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--steps", default=",".join(STEPS), help="comma-separated steps to run")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "group-wise weight scales (nqk_qgemm_group) against nqk_qgemm_i8 + nqk_dequantize_cols",
              "rounds": args.rounds}
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}"
                   for k in ("gemm_batch", "model_batch", "model_batch_large", "rounds", "warmup", "reps")]
    for name in args.steps.split(","):
        limit = STEPS[name][1]
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_group] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_group] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
