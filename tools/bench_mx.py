#!/usr/bin/env python
"""MX operands (nqk_quantize_mx, nqk_gemm_mx) on one MI355X.  Prints one JSON line (and writes it to
--out, e.g. profiles/mx.json).

  gemm    ViT-Base's four projection shapes at --gemm-batch images: kernels.gemm_mx at the three
          format pairs beside kernels.qmatmul_rows (its integer counterpart) and nqk_qgemm_i8 followed
          by nqk_dequantize_cols; the MX legs also as a share of the FP8 matrix peak (the FP4 peak,
          twice that, for fp4 x fp4)
  quant   kernels.quantize_mx at both formats on [M, 768] and [M, 3072] float32 beside
          kernels.quantize_rows and a device-to-device copy of the same array: bytes per second as a
          fraction of the copy's
  model   the node-loop forward of ViT-Base (synthetic weights), per_channel, at mxfp8, (mxfp8, mxfp4)
          and mxfp4 beside per_token=True, at every batch of --model-batches
  error   model.compare's output MSE and SQNR on the three encoder-layer fixtures of
          tools/bench_per_token.py at the three MX cells beside per-tensor (8, 8) and (8, 4), per_channel

The legs of a step alternate in one process; a figure is the median of its --rounds windows, with
min-max.  Each GPU step is a child process under its own time limit; after a step that fails or runs
out of time nothing more is started.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "numpy-quant_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from bench_per_token import MODELS, SHAPES, T, D, TOKEN_FACTOR, TOKEN_ROWS, _alternate  # noqa: E402

FP8_PEAK_OPS = 256 * 2.4e9 * 8192  # dense FP8 MFMA operations per second (the int8 rate); FP4 issues at twice it
MX_CELLS = {"mxfp8": ("mxfp8", "mxfp8"), "mxfp8_w4": ("mxfp8", "mxfp4"), "mxfp4": ("mxfp4", "mxfp4")}


def _put(res, key, stats):
    for leg, (med, span, _) in stats.items():
        res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = med, span


def step_gemm(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rng = np.random.default_rng(16)
    M = args.gemm_batch * T
    res = {"gemm_batch": args.gemm_batch, "gemm_M": M}
    for name, (Kd, N) in SHAPES.items():
        x = DeviceArray.from_host(rng.standard_normal((M, Kd)).astype(np.float32))
        wt = DeviceArray.from_host(rng.standard_normal((N, Kd)).astype(np.float32))
        mx = {f: (K.quantize_mx(x, f), K.quantize_mx(wt, f)) for f in K.MX_FORMATS}
        a = DeviceArray.from_host(rng.integers(-128, 128, size=(M, Kd), dtype=np.int8))
        b = DeviceArray.from_host(rng.integers(-128, 128, size=(Kd, N), dtype=np.int8))
        bt, col = K.weight_bt(b)
        sw = DeviceArray.from_host(np.exp2(rng.uniform(-12, -8, size=N)).astype(np.float32))
        rq = K.RowQuantized(a, DeviceArray.from_host(np.exp2(rng.uniform(-6, -2, size=M)).astype(np.float32)),
                            DeviceArray.from_host(rng.integers(-128, 128, size=M).astype(np.int32)), (M, Kd), 8)

        def i8_dequant():
            acc, zt = K.qmatmul(a, b, 3, None, bt, col)
            return K.dequantize_cols(acc, sw, zt)
        legs = {cell: (lambda fa=fa, fb=fb: K.gemm_mx(mx[fa][0], mx[fb][1])) for cell, (fa, fb) in MX_CELLS.items()}
        legs.update(rows=lambda: K.qmatmul_rows(rq, bt, col, sw), i8_dequant=i8_dequant)
        stats = _alternate(legs, args, args.reps)
        key = f"gemm_{name}"
        _put(res, key, stats)
        for cell in MX_CELLS:
            res[f"{key}_{cell}_over_rows"] = round(stats[cell][0] / stats["rows"][0], 3)
            peak = FP8_PEAK_OPS * (2 if cell == "mxfp4" else 1)
            res[f"{key}_{cell}_peak_share"] = round(2 * M * N * Kd / (stats[cell][0] * 1e-3) / peak, 4)
    return res


def step_quant(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rng = np.random.default_rng(17)
    M = args.gemm_batch * T
    res = {}
    for cols in (D, 4 * D):
        x = DeviceArray.from_host(rng.standard_normal((M, cols)).astype(np.float32))
        stats = _alternate({"mxfp8": lambda: K.quantize_mx(x, "mxfp8"), "mxfp4": lambda: K.quantize_mx(x, "mxfp4"),
                            "rows": lambda: K.quantize_rows(x, 8), "copy": x.copy}, args, args.reps)
        key = f"quant_{cols}"
        _put(res, key, stats)
        copy_rate = 8 / stats["copy"][0]
        for leg, bpe in (("mxfp8", 5 + 1 / 32), ("mxfp4", 4.5 + 1 / 32), ("rows", 5)):
            res[f"{key}_{leg}_fraction_of_copy_rate"] = round(bpe / stats[leg][0] / copy_rate, 3)
        res[f"{key}_copy_tb_per_s"] = round(8 * M * cols / (stats["copy"][0] * 1e-3) / 1e12, 3)
    return res


def step_model(args) -> dict:
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    res = {}
    for B in args.model_batches:
        x = np.random.default_rng(12345).standard_normal((B, 3, 224, 224)).astype(np.float32)
        proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
        onnx_proto.rebatch(proto, B)
        model = Model.from_onnx(proto)
        qs = {cell: model.quantize([x], per_channel=True, mx_format=fa, mx_weight_format=fb)
              for cell, (fa, fb) in MX_CELLS.items()}
        qs["per_token"] = model.quantize([x], per_channel=True, per_token=True)
        for q in qs.values():
            q.keep_values = True  # the node loop on every leg
        stats = _alternate({leg: (lambda q=q: q([x])) for leg, q in qs.items()}, args, 1, 2)
        _put(res, f"model_b{B}", stats)
        for cell in MX_CELLS:
            res[f"model_b{B}_{cell}_over_per_token"] = round(stats[cell][0] / stats["per_token"][0], 3)
        del qs, model
    return res


def step_error(args) -> dict:
    from numpy_quant.model import Model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _equalize_ref as E
    import _perchannel_ref as P
    proto, _, xs = P.encoder_layer_fixture(MODELS)
    oproto, _, xo, _ = E.outlier_fixture(MODELS)
    xt = xs.copy()
    xt[:, TOKEN_ROWS, :] *= np.float32(TOKEN_FACTOR)
    fixtures = {"spread_columns": (Model.from_onnx(proto), xs),
                "equalized_outliers": (Model.from_onnx(oproto).equalize([[xo]]), xo),
                "outlier_tokens": (Model.from_onnx(proto), xt)}
    cells = {cell: dict(mx_format=fa, mx_weight_format=fb) for cell, (fa, fb) in MX_CELLS.items()}
    cells.update(a8w8={}, a8w4={"weight_bit_width": 4})
    res = {}
    for fixture, (model, x) in fixtures.items():
        out = model.outputs[0].name
        for cell, kw in cells.items():
            s = model.compare(model.quantize([x], bit_width=8, per_channel=True, **kw), [[x]], k=1).values[out]
            res[f"error_{fixture}_{cell}_mse"] = float(s.mse)
            res[f"error_{fixture}_{cell}_sqnr_db"] = round(float(s.sqnr_db), 3)
    return res


STEPS = {"gemm": (step_gemm, 200), "quant": (step_quant, 120), "model": (step_model, 500), "error": (step_error, 300)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gemm-batch", type=int, default=64, help="images behind the GEMM and quantizer shapes")
    ap.add_argument("--model-batches", type=lambda s: [int(v) for v in s.split(",")], default=[8, 64],
                    help="images of the node-loop forwards, comma-separated")
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
    result = {"metric": "MX operands (nqk_quantize_mx, nqk_gemm_mx) against the int8 routes", "rounds": args.rounds}
    passthrough = [f"--gemm-batch={args.gemm_batch}", "--model-batches=" + ",".join(map(str, args.model_batches)),
                   f"--rounds={args.rounds}", f"--warmup={args.warmup}", f"--reps={args.reps}"]
    for name in args.steps.split(","):
        limit = STEPS[name][1]
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_mx] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_mx] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
