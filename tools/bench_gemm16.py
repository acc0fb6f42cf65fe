#!/usr/bin/env python
"""nqk_qgemm_i16 (9..16-bit activations as byte planes on the int8 MFMAs) against the route it
replaces, nqk_qgemm_generic, on one MI355X.  Prints one JSON line (and writes it to --out, e.g.
profiles/gemm16.json).

  gemm    kernels.qmatmul on ViT-Base's four projection shapes (constant weight, its Bt cached) and
          the two attention products (both operands activations), int16 x int8 and int16 x int16,
          at --gemm-batch images: the new route and the NQK_GEMM16=0 leg alternate, each checked
          against the other bit for bit.  The kernel alone (KernelTimer, "qgemm_i16") gives the
          share of the int8 MFMA peak: all byte-plane products over the peak, and the useful
          product (that figure over the 2 or 4 plane products)
  model   the node-loop forward of ViT-Base (synthetic weights) at (16, 8) and (16, 16), with and
          without NQK_GEMM16=0, logits compared bit for bit
  error   model.compare's output MSE on the encoder-layer fixture at (8, 8), (16, 8), (16, 16)

With --epi the steps are those of nqk_qgemm_i16_epi instead (e.g. --out profiles/gemm16_epi.json); the
reference is the parent's route, which NQK_GEMM16_EPI=0 keeps:

  epi_gemm   per product above: nqk_qgemm_i16 + nqk_dequantize (two launches, the int64 array between
             them) against the one fused launch, compared bit for bit; the fused kernel alone gives
             the bytes per second it achieves (operands read once + the f32 output)
  epi_model  the node-loop forward of ViT-Base at (16, 8) and (16, 16), at --model-batch and at
             --model-batch-large images, with and without NQK_GEMM16_EPI=0, logits compared bit for bit

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
T, D, H = 197, 768, 12
# name: (batch dims of a per image, M, K, N, b is a constant weight)
SHAPES = {"qkv": (None, T, D, 3 * D, True), "out_proj": (None, T, D, D, True), "ffn_up": (None, T, D, 4 * D, True),
          "ffn_down": (None, T, 4 * D, D, True), "scores": (H, T, D // H, T, False), "pv": (H, T, T, D // H, False)}
LEGS = (("i16", "1"), ("generic", "0"))


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
    B = args.gemm_batch
    res = {"gemm_batch": B}
    for name, (heads, M, Kd, N, const) in SHAPES.items():
        for wb, bdt in ((8, np.int8), (16, np.int16)):
            if heads is None:  # the images' rows are one matrix
                ash, bsh = (B * M, Kd), (Kd, N)
            else:
                ash, bsh = (B, heads, M, Kd), (B, heads, Kd, N)
            a = DeviceArray.from_host(rng.integers(-32768, 32768, size=ash).astype(np.int16))
            b = DeviceArray.from_host(rng.integers(np.iinfo(bdt).min, np.iinfo(bdt).max + 1, size=bsh).astype(bdt))
            bt, col = K.weight_bt(b) if const else (None, None)
            call = lambda: K.qmatmul(a, b, None, None, bt, col)
            outs = {}
            for leg, env in LEGS:
                os.environ["NQK_GEMM16"] = env
                outs[leg] = call()[0].to_host()
            if not np.array_equal(outs["i16"], outs["generic"]):
                raise AssertionError(f"{name} w{wb}: the two routes differ")
            samples = {leg: [] for leg, _ in LEGS}
            for i in range(args.warmup + args.rounds):
                for leg, env in LEGS:
                    os.environ["NQK_GEMM16"] = env
                    ms = _timer_ms(lambda: [call() for _ in range(args.reps)]) / args.reps
                    if i >= args.warmup:
                        samples[leg].append(ms)
            key = f"gemm_{name}_a16w{wb}"
            for leg, _ in LEGS:
                res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = _stats(samples[leg])
            res[f"{key}_speedup"] = round(res[f"{key}_generic_ms"] / res[f"{key}_i16_ms"], 2)
            # the kernel alone
            os.environ["NQK_GEMM16"] = "1"
            K.TIMER = K.KernelTimer()
            for _ in range(args.rounds):
                call()
            K.qmatmul(a, b, None, None, bt, col)[0].to_host()  # a synchronising call: every event has passed
            recs = [r for r in K.TIMER.collect() if r[0] == "qgemm_i16"]
            K.TIMER = None
            ms = statistics.median(r[1] for r in recs)
            planes = 2 * wb // 8
            share = recs[0][2][0] / (ms * 1e-3) / INT8_PEAK_OPS
            res[f"{key}_kernel_ms"] = round(ms, 4)
            res[f"{key}_mfma_peak_share"] = round(share, 4)
            res[f"{key}_useful_peak_share"] = round(share / planes, 4)
    os.environ.pop("NQK_GEMM16", None)
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
    for wbw in (8, 16):
        q = model.quantize([x], bit_width=16, weight_bit_width=wbw)
        logits = {}
        for leg, env in LEGS:
            os.environ["NQK_GEMM16"] = env
            logits[leg] = q([x])[0]
        if not np.array_equal(logits["i16"].view(np.uint32), logits["generic"].view(np.uint32)):
            raise AssertionError(f"(16, {wbw}): the two routes give different logits")
        samples = {leg: [] for leg, _ in LEGS}
        for i in range(args.warmup + args.rounds):
            for leg, env in LEGS:
                os.environ["NQK_GEMM16"] = env
                ms = _timer_ms(lambda: q([x]))
                if i >= args.warmup:
                    samples[leg].append(ms)
        key = f"model_a16w{wbw}"
        for leg, _ in LEGS:
            res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = _stats(samples[leg], 2)
        res[f"{key}_speedup"] = round(res[f"{key}_generic_ms"] / res[f"{key}_i16_ms"], 2)
        res[f"{key}_ranges_overlap"] = bool(max(samples["i16"]) >= min(samples["generic"]))
    os.environ.pop("NQK_GEMM16", None)
    return res


EPI_LEGS = (("fused", "1"), ("two_launch", "0"))


def step_epi_gemm(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray
    rng = np.random.default_rng(16)
    B, scale = args.gemm_batch, np.float32(3.1e-7)
    res = {"gemm_batch": B}
    for name, (heads, M, Kd, N, const) in SHAPES.items():
        for wb, bdt in ((8, np.int8), (16, np.int16)):
            if heads is None:
                ash, bsh = (B * M, Kd), (Kd, N)
            else:
                ash, bsh = (B, heads, M, Kd), (B, heads, Kd, N)
            a = DeviceArray.from_host(rng.integers(-32768, 32768, size=ash).astype(np.int16))
            b = DeviceArray.from_host(rng.integers(np.iinfo(bdt).min, np.iinfo(bdt).max + 1, size=bsh).astype(bdt))
            bt, col = K.weight_bt(b) if const else (None, None)

            def call():  # what QTensor.matmul(...).dequantize() launches on either leg
                acc = K.qmatmul(a, b, None, None, bt, col, defer=True)[0]
                return acc.dequantize(scale) if isinstance(acc, K.PendingProduct) else K.dequantize(acc, scale, None)
            outs = {}
            for leg, env in EPI_LEGS:
                os.environ["NQK_GEMM16_EPI"] = env
                outs[leg] = call().to_host()
            if outs["fused"].tobytes() != outs["two_launch"].tobytes():
                raise AssertionError(f"{name} w{wb}: the fused launch and the two launches differ")
            samples = {leg: [] for leg, _ in EPI_LEGS}
            for i in range(args.warmup + args.rounds):
                for leg, env in EPI_LEGS:
                    os.environ["NQK_GEMM16_EPI"] = env
                    ms = _timer_ms(lambda: [call() for _ in range(args.reps)]) / args.reps
                    if i >= args.warmup:
                        samples[leg].append(ms)
            key = f"epi_{name}_a16w{wb}"
            for leg, _ in EPI_LEGS:
                res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = _stats(samples[leg])
            res[f"{key}_speedup"] = round(res[f"{key}_two_launch_ms"] / res[f"{key}_fused_ms"], 2)
            res[f"{key}_ranges_overlap"] = bool(max(samples["fused"]) >= min(samples["two_launch"]))
            os.environ["NQK_GEMM16_EPI"] = "1"
            K.TIMER = K.KernelTimer()
            for _ in range(args.rounds):
                call()
            call().to_host()  # a synchronising call: every event has passed
            recs = [r for r in K.TIMER.collect() if r[0] == "qgemm_i16"]
            K.TIMER = None
            ms = statistics.median(r[1] for r in recs)
            res[f"{key}_kernel_ms"] = round(ms, 4)
            res[f"{key}_kernel_bytes"] = int(recs[0][2][1])
            res[f"{key}_kernel_tb_per_s"] = round(recs[0][2][1] / (ms * 1e-3) / 1e12, 3)
    os.environ.pop("NQK_GEMM16_EPI", None)
    return res


def step_epi_model(args) -> dict:
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    res = {"model_batches": [args.model_batch, args.model_batch_large]}
    for B in res["model_batches"]:
        x = np.random.default_rng(12345).standard_normal((B, 3, 224, 224)).astype(np.float32)
        proto = onnx_proto.load(os.path.join(MODELS, "vit_image_classifier_no_weights.onnx"), synthetic_weights=True)
        onnx_proto.rebatch(proto, B)
        model = Model.from_onnx(proto)
        for wbw in (8, 16):
            q = model.quantize([x], bit_width=16, weight_bit_width=wbw)
            logits = {}
            for leg, env in EPI_LEGS:
                os.environ["NQK_GEMM16_EPI"] = env
                logits[leg] = q([x])[0]
            if logits["fused"].tobytes() != logits["two_launch"].tobytes():
                raise AssertionError(f"(16, {wbw}) at {B} images: the two routes give different logits")
            samples = {leg: [] for leg, _ in EPI_LEGS}
            for i in range(args.warmup + args.rounds):
                for leg, env in EPI_LEGS:
                    os.environ["NQK_GEMM16_EPI"] = env
                    ms = _timer_ms(lambda: q([x]))
                    if i >= args.warmup:
                        samples[leg].append(ms)
            key = f"epi_model_b{B}_a16w{wbw}"
            for leg, _ in EPI_LEGS:
                res[f"{key}_{leg}_ms"], res[f"{key}_{leg}_ms_min_max"] = _stats(samples[leg], 2)
            res[f"{key}_speedup"] = round(res[f"{key}_two_launch_ms"] / res[f"{key}_fused_ms"], 3)
            res[f"{key}_ranges_overlap"] = bool(max(samples["fused"]) >= min(samples["two_launch"]))
            del q
    os.environ.pop("NQK_GEMM16_EPI", None)
    return res


def step_error(args) -> dict:
    from numpy_quant.model import Model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _perchannel_ref as R
    proto, _, x = R.encoder_layer_fixture(MODELS, seed=R.SEED, batch=2)
    model = Model.from_onnx(proto)
    out = model.outputs[0].name
    res = {}
    for bw, wbw in ((8, 8), (16, 8), (16, 16)):
        s = model.compare(model.quantize([x], bit_width=bw, weight_bit_width=wbw), [[x]], k=1).values[out]
        res[f"error_a{bw}w{wbw}_output_mse"] = float(s.mse)
        res[f"error_a{bw}w{wbw}_output_sqnr_db"] = round(float(s.sqnr_db), 3)
    return res


STEPS = {"gemm": (step_gemm, 300), "model": (step_model, 420), "error": (step_error, 240)}
EPI_STEPS = {"epi_gemm": (step_epi_gemm, 300), "epi_model": (step_epi_model, 600)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gemm-batch", type=int, default=8, help="images behind the GEMM shapes")
    ap.add_argument("--model-batch", type=int, default=8, help="images of the node-loop forward")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="qmatmul calls per timed window")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--model-batch-large", type=int, default=64, help="the second batch of --epi's forward")
    ap.add_argument("--epi", action="store_true", help="measure nqk_qgemm_i16_epi against the two-launch route instead")
    ap.add_argument("--step", choices=sorted({**STEPS, **EPI_STEPS}), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps({**STEPS, **EPI_STEPS}[args.step][0](args)), flush=True)
        return 0
    metric = ("the fused dequantize / requantize epilogue (nqk_qgemm_i16_epi) against nqk_qgemm_i16 and a second launch"
              if args.epi else "int16 activations on the int8 MFMAs (nqk_qgemm_i16) against nqk_qgemm_generic")
    result = {"metric": metric, "rounds": args.rounds}
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}"
                   for k in ("gemm_batch", "model_batch", "model_batch_large", "rounds", "warmup", "reps")]
    for name, (_, limit) in (EPI_STEPS if args.epi else STEPS).items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_gemm16] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_gemm16] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
