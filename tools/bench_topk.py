#!/usr/bin/env python
"""Top-k classes and probabilities at the headline shape (ViT-Base int8, B=256, synthetic
weights), float32 host arrays in, on one MI355X.  Prints one JSON line.

  classify   qmodel.classify([x], 5): the top-k kernel reads the quantized logits on the device,
             [B, 5] indices and probabilities come back
  baseline   qmodel([x]) followed by NumPy on the host: softmax, stable argsort, slice (the only
             way to the same answer without the kernel)
and, with the library's stream timer (device events): nqk_topk_softmax alone on [256, 1000] int8
and f32, and on [50 432, 1000] f32 rotating over buffers larger than the 256 MiB Infinity Cache
together, as rows x cols x element size over the time beside the device copy rate; on that shape
also its parts (probabilities off, k = 1, k = 64) and nqk_softmax_lastdim for scale.

Every row of `classify` is compared with the baseline's (bit for bit) before anything is
reported.  The two legs are timed in alternating rounds in one process; the figure of a leg is
the median of its rounds.  Each GPU step is a child process under its own time limit; after a
step that fails or runs out of time nothing more is started.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "numpy-quant_amd"), ROOT):
    sys.path.insert(0, p)

COPY_RATE = 6.29e12  # B/s, the device copy rate DESIGN.md quotes
MODEL_FILE = os.path.join(ROOT, "numpy-quant_amd", "models", "vit_image_classifier_no_weights.onnx")
BIG_ROWS = 50432     # 256 images x 197 tokens: the row count of the model's largest row kernels


def host_topk(logits, k):
    """the three NumPy lines"""
    e = np.exp(logits + (-logits.max(-1, keepdims=True)))
    p = e / e.sum(-1, keepdims=True)
    idx = np.argsort(-logits, axis=-1, kind="stable")[:, :k]
    return idx, np.take_along_axis(p, idx, -1)


def _timer_ms(fn) -> float:
    from numpy_quant import _lib
    _lib.call("nqk_timer_start")
    fn()
    _lib.call("nqk_timer_stop")
    ms = ctypes.c_float()
    _lib.call("nqk_timer_ms", ctypes.byref(ms))
    return ms.value


def step_micro(args) -> dict:
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray, sync
    _lib.ensure_init()
    rng = np.random.default_rng(2026)
    k, cols = args.k, 1000
    res = {}
    shapes = [("i8_256", args.batch, np.int8), ("f32_256", args.batch, np.float32), ("f32_big", BIG_ROWS, np.float32)]
    for name, rows, dtype in shapes:
        nbytes = rows * cols * np.dtype(dtype).itemsize
        copies = max(1, -(-(320 << 20) // nbytes)) if rows == BIG_ROWS else 1  # more than 256 MiB in flight
        if dtype == np.int8:
            host = rng.integers(-128, 128, size=(rows, cols)).astype(np.int8)
            scale, zp = np.float32(0.07), -5
            y = (host.astype(np.int64) - zp).astype(np.float64) * np.float64(scale)
            y = y.astype(np.float32)
        else:
            host = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
            scale = zp = None
            y = host
        srcs = [DeviceArray.from_host(host) for _ in range(copies)]
        idx, prob, _ = K.topk_softmax(srcs[0], k, scale=scale, zp=zp)
        want_idx, want_prob = host_topk(y, k)
        if not (np.array_equal(idx.to_host(), want_idx)
                and np.array_equal(prob.to_host().view(np.uint32), want_prob.view(np.uint32))):
            raise AssertionError(f"nqk_topk_softmax differs from NumPy on {name}")
        args_c = (float(np.float32(1.0 if scale is None else scale)), 0 if zp is None else zp, 0 if zp is None else 1,
                  rows, cols, cols, k, idx.vp, prob.vp, None)

        def kernel_round():
            for s in srcs:
                _lib.call("nqk_topk_softmax", s.vp, s.code, *args_c)

        samples = []
        for i in range(args.warmup + args.rounds):
            ms = _timer_ms(lambda: [kernel_round() for _ in range(args.reps)])
            if i >= args.warmup:
                samples.append(1e3 * ms / (args.reps * copies))
        us = statistics.median(samples)
        res[f"topk_{name}_us"] = round(us, 2)
        res[f"topk_{name}_us_min_max"] = [round(min(samples), 2), round(max(samples), 2)]
        if rows == BIG_ROWS:
            # the parts of that time: without the probabilities, one round only, 64 rounds, and the
            # library's own Softmax over the same rows for scale
            out = DeviceArray((rows, cols), np.float32)
            idx64, prob64 = DeviceArray((rows, 64), np.int64), DeviceArray((rows, 64), np.float32)
            variants = {
                "k5_noprob": lambda s: _lib.call("nqk_topk_softmax", s.vp, s.code, 1.0, 0, 0, rows, cols, cols, k,
                                                 idx.vp, None, None),
                "k1_noprob": lambda s: _lib.call("nqk_topk_softmax", s.vp, s.code, 1.0, 0, 0, rows, cols, cols, 1,
                                                 idx64.vp, None, None),
                "k64": lambda s: _lib.call("nqk_topk_softmax", s.vp, s.code, 1.0, 0, 0, rows, cols, cols, 64,
                                           idx64.vp, prob64.vp, None),
                "softmax_lastdim": lambda s: _lib.call("nqk_softmax_lastdim", s.vp, out.vp, rows, cols),
            }
            for vname, fn in variants.items():
                vs = []
                for i in range(args.warmup + args.rounds):
                    ms = _timer_ms(lambda: [fn(s) for _ in range(args.reps) for s in srcs])
                    if i >= args.warmup:
                        vs.append(1e3 * ms / (args.reps * copies))
                res[f"big_{vname}_us"] = round(statistics.median(vs), 2)
            res["topk_f32_big_rows"] = rows
            res["topk_f32_big_bytes"] = nbytes
            res["topk_f32_big_buffers"] = copies
            res["topk_f32_big_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
            res["topk_f32_big_fraction_of_copy_rate"] = round(nbytes / (us * 1e-6) / COPY_RATE, 3)
        sync()
    return res


def step_e2e(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.model import Model
    _lib.ensure_init()
    B, k = args.batch, args.k
    rng = np.random.default_rng(2024)
    xs = [rng.standard_normal((B, 3, 224, 224)).astype(np.float32) for _ in range(args.batches)]
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    calib = min(8, B)
    model.rebatch(calib)
    qmodel = model.quantize([xs[0][:calib]], bit_width=8)
    for v in model.values:  # free the float calibration activations
        if v.__class__.__name__ == "Variable":
            v.data = None
    model.rebatch(B)
    plan = qmodel.compile()

    rows = 0
    for x in xs:
        want_idx, want_prob = host_topk(qmodel([x])[0], k)
        idx, prob = qmodel.classify([x], k)
        if not (np.array_equal(idx, want_idx) and np.array_equal(prob.view(np.uint32), want_prob.view(np.uint32))):
            raise AssertionError("qmodel.classify differs from qmodel() + NumPy")
        rows += idx.shape[0]

    def leg_classify():
        for x in xs:
            qmodel.classify([x], k)

    def leg_baseline():
        for x in xs:
            host_topk(qmodel([x])[0], k)

    def leg_forward_only():
        for x in xs:
            qmodel([x])

    legs = {"classify": leg_classify, "baseline": leg_baseline, "forward_only": leg_forward_only}
    samples = {name: [] for name in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():  # alternating: the same box, the same minutes
            t0 = time.perf_counter()
            fn()  # every call ends in a synchronous read-back
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0) / len(xs))
    # the host's share of the baseline: the three NumPy lines alone
    logits = qmodel([xs[0]])[0]
    host = []
    for _ in range(args.warmup + args.rounds):
        t0 = time.perf_counter()
        host_topk(logits, k)
        host.append(1e3 * (time.perf_counter() - t0))
    res = {"fused_layers": plan.fused, "rows_verified": rows,
           "host_numpy_topk_ms": round(statistics.median(host[args.warmup:]), 3)}
    for name, s in samples.items():
        res[f"{name}_ms_per_batch"] = round(statistics.median(s), 3)
        res[f"{name}_ms_min_max"] = [round(min(s), 3), round(max(s), 3)]
        res[f"{name}_images_per_s"] = round(B / (statistics.median(s) * 1e-3), 1)
    return res


STEPS = {"micro": (step_micro, 240), "e2e": (step_e2e, 420)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="kernel launches per buffer and timed window")
    ap.add_argument("--batches", type=int, default=2, help="distinct input batches per timed round")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "top-k classes and probabilities, ViT-Base int8 (synthetic weights), float32 host arrays in",
              "batch": args.batch, "k": args.k, "rounds": args.rounds, "batches": args.batches,
              "verified": "every row of classify equals qmodel() + NumPy softmax / stable argsort, bit for bit"}
    passthrough = [f"--{name}={getattr(args, name)}" for name in ("batch", "k", "rounds", "warmup", "reps", "batches")]
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_topk] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_topk] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
            return p.returncode or 1
        result.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
