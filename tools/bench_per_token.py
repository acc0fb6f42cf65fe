#!/usr/bin/env python
"""Per-token activation scales (nqk_quantize_rows, nqk_qgemm_rows) on one MI355X.  Prints one JSON
line (and writes it to --out, e.g. profiles/per_token.json).

  gemm    ViT-Base's four projection shapes at --gemm-batch images: kernels.qmatmul_rows beside
          nqk_qgemm_i8 followed by nqk_dequantize_cols on the same integers (the per-tensor
          activation route; not the same result)
  quant   kernels.quantize_rows on [M, 768] and [M, 3072] float32 beside kernels.quantize (one
          calibrated scale), and a device-to-device copy of the same array: the quantizer's bytes
          per second (4 in + 1 out per element) as a fraction of the copy's (4 in + 4 out)
  model   the node-loop forward of ViT-Base (synthetic weights) at (8, 8) and (8, 4), per_channel,
          with and without per_token, at --model-batch images
  error   model.compare's output MSE and SQNR, with and without per_token, at (8, 8) and (8, 4)
          per_channel, on three encoder-layer fixtures: spread weight columns, equalized LayerNorm
          outlier channels, and the first with a few token rows of the input multiplied by 32

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
T, D = 197, 768
SHAPES = {"qkv": (D, 3 * D), "out_proj": (D, D), "ffn_up": (D, 4 * D), "ffn_down": (4 * D, D)}  # name: (K, N)
CELLS = {"a8w8": {}, "a8w4": {"weight_bit_width": 4}}
TOKEN_ROWS, TOKEN_FACTOR = (0, 17, 101), 32.0


def _timer_ms(fn) -> float:
    from numpy_quant import _lib
    _lib.call("nqk_timer_start")
    fn()
    _lib.call("nqk_timer_stop")
    ms = ctypes.c_float()
    _lib.call("nqk_timer_ms", ctypes.byref(ms))
    return ms.value


def _alternate(legs, args, reps, digits=4):
    """{leg: (median ms, [min, max], samples)} of one call, the legs alternating window by window."""
    samples = {leg: [] for leg in legs}
    for i in range(args.warmup + args.rounds):
        for leg, call in legs.items():
            ms = _timer_ms(lambda: [call() for _ in range(reps)]) / reps
            if i >= args.warmup:
                samples[leg].append(ms)
    return {leg: (round(statistics.median(v), digits), [round(min(v), digits), round(max(v), digits)], v)
            for leg, v in samples.items()}


def _record(res, key, stats, a, b):
    for leg, (med, span, _) in stats.items():
        res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = med, span
    res[f"{key}_ratio"] = round(stats[a][0] / stats[b][0], 3)
    res[f"{key}_ranges_overlap"] = bool(max(stats[a][2]) >= min(stats[b][2]) and max(stats[b][2]) >= min(stats[a][2]))


def step_gemm(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rng = np.random.default_rng(16)
    M = args.gemm_batch * T
    res = {"gemm_batch": args.gemm_batch, "gemm_M": M}
    for name, (Kd, N) in SHAPES.items():
        a = DeviceArray.from_host(rng.integers(-128, 128, size=(M, Kd), dtype=np.int8))
        b = DeviceArray.from_host(rng.integers(-128, 128, size=(Kd, N), dtype=np.int8))
        bt, col = K.weight_bt(b)
        sw = DeviceArray.from_host(np.exp2(rng.uniform(-12, -8, size=N)).astype(np.float32))
        rq = K.RowQuantized(a, DeviceArray.from_host(np.exp2(rng.uniform(-6, -2, size=M)).astype(np.float32)),
                            DeviceArray.from_host(rng.integers(-128, 128, size=M).astype(np.int32)), (M, Kd), 8)

        def i8_dequant():
            acc, zt = K.qmatmul(a, b, 3, None, bt, col)
            return K.dequantize_cols(acc, sw, zt)
        stats = _alternate({"rows": lambda: K.qmatmul_rows(rq, bt, col, sw), "i8_dequant": i8_dequant}, args, args.reps)
        _record(res, f"gemm_{name}", stats, "rows", "i8_dequant")
    return res


def step_quant(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rng = np.random.default_rng(17)
    M = args.gemm_batch * T
    res = {}
    for cols in (D, 4 * D):
        x = DeviceArray.from_host(rng.standard_normal((M, cols)).astype(np.float32))
        stats = _alternate({"rows": lambda: K.quantize_rows(x, 8), "scalar": lambda: K.quantize(x, 8, 0.03, 5),
                            "copy": x.copy}, args, args.reps)
        key = f"quant_{cols}"
        _record(res, key, stats, "rows", "scalar")
        rate = {leg: bpe * M * cols / (stats[leg][0] * 1e-3) for leg, bpe in (("rows", 5), ("scalar", 5), ("copy", 8))}
        res[f"{key}_rows_tb_per_s"] = round(rate["rows"] / 1e12, 3)
        res[f"{key}_copy_tb_per_s"] = round(rate["copy"] / 1e12, 3)
        res[f"{key}_rows_fraction_of_copy_rate"] = round(rate["rows"] / rate["copy"], 3)
        res[f"{key}_scalar_fraction_of_copy_rate"] = round(rate["scalar"] / rate["copy"], 3)
    return res


def step_model(args) -> dict:
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    B = args.model_batch
    x = np.random.default_rng(12345).standard_normal((B, 3, 224, 224)).astype(np.float32)
    proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
    onnx_proto.rebatch(proto, B)
    model = Model.from_onnx(proto)
    res = {"model_batch": B}
    for cell, kw in CELLS.items():
        qs = {leg: model.quantize([x], bit_width=8, per_channel=True, per_token=flag, **kw)
              for leg, flag in (("per_token", True), ("per_tensor", False))}
        for q in qs.values():
            q.keep_values = True  # the node loop on both legs
        stats = _alternate({leg: (lambda q=q: q([x])) for leg, q in qs.items()}, args, 1, 2)
        _record(res, f"model_b{B}_{cell}", stats, "per_token", "per_tensor")
        del qs
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
    res = {"outlier_token_rows": list(TOKEN_ROWS), "outlier_token_factor": TOKEN_FACTOR}
    for fixture, (model, x) in fixtures.items():
        out = model.outputs[0].name
        for cell, kw in CELLS.items():
            for leg, flag in (("per_token", True), ("per_tensor", False)):
                q = model.quantize([x], bit_width=8, per_channel=True, per_token=flag, **kw)
                s = model.compare(q, [[x]], k=1).values[out]
                res[f"error_{fixture}_{cell}_{leg}_mse"] = float(s.mse)
                res[f"error_{fixture}_{cell}_{leg}_sqnr_db"] = round(float(s.sqnr_db), 3)
    return res


STEPS = {"gemm": (step_gemm, 200), "quant": (step_quant, 120), "model": (step_model, 400), "error": (step_error, 300)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gemm-batch", type=int, default=64, help="images behind the GEMM and quantizer shapes")
    ap.add_argument("--model-batch", type=int, default=8, help="images of the node-loop forward")
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
    result = {"metric": "per-token activation scales (nqk_quantize_rows, nqk_qgemm_rows) against one calibrated scale",
              "rounds": args.rounds}
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("gemm_batch", "model_batch", "rounds", "warmup", "reps")]
    for name in args.steps.split(","):
        limit = STEPS[name][1]
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_per_token] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_per_token] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
