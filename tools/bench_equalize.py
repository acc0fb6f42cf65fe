#!/usr/bin/env python
"""Channel equalization (Model.equalize) on one MI355X.  Prints one JSON line (and writes it to
--out, e.g. profiles/equalize.json).

  kernel  nqk_absmax_f32 alone, library stream timer: axis 0 on float32 [50432, 768] and
          [50432, 3072], axis 1 on [768, 3072], rotating over more than 256 MiB of buffers; beside
          it nqk_hist_f32's range-only pass (counts = 0) and a device-to-device copy of the same
          arrays: us, TB/s read, and the fraction of the copy rate
  cost    ViT-Base (synthetic weights), 8 calibration images: wall time of model.equalize against
          model.calibrate_stream on the same batch, and the float forward alone
  error   the tests' outlier fixture (tests/_equalize_ref.outlier_fixture: the encoder layer, 6 of 768
          entries of each LayerNorm's gamma times 32), batch 2: model.compare's output MSE and SQNR at
          (8, 8), (8, 8) per column, (8, 4) per column and (4, 4), plain and equalized with alpha in
          {0.25, 0.5, 0.75}, the SQNR of the LN outputs and of the site weights; and the same on the
          stand-in weights without outliers
  step    the graph-replayed ViT-Base forward at B = 256, int8, plain against equalized, and the four
          projection GEMMs' kernel times of a plain forward of each

The legs of a step alternate in one process; a figure is the median of its --rounds windows, with
min-max.  Each GPU step is a child process under its own time limit; after a step that fails or
runs out of time nothing more is started.
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

MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
MODEL_FILE = os.path.join(MODELS, "vit_image_classifier_no_weights.onnx")
COPY_RATE = 6.29e12  # B/s, the device copy rate DESIGN.md quotes
BIG_ROWS = 50432     # 256 images x 197 tokens


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


def step_kernel(args) -> dict:
    from numpy_quant import _lib
    from numpy_quant import calibration as C
    from numpy_quant.device import DeviceArray, sync
    _lib.ensure_init()
    rng = np.random.default_rng(2028)
    res = {}
    for rows, cols, axis in ((BIG_ROWS, 768, 0), (BIG_ROWS, 3072, 0), (768, 3072, 1)):
        nbytes = rows * cols * 4
        copies = max(2, -(-(320 << 20) // nbytes))  # more than 256 MiB in flight
        copies = min(copies, 64)
        host = rng.standard_normal((rows, cols), dtype=np.float32)
        srcs = [DeviceArray.from_host(host) for _ in range(copies)]
        dst = DeviceArray((rows, cols), np.float32)
        n = cols if axis == 0 else rows
        state = DeviceArray((n,), np.uint32).fill_zero()
        hstate = DeviceArray.from_host(C.fresh_state())
        _lib.call("nqk_absmax_f32", srcs[0].vp, rows, cols, cols, axis, state.vp)
        if not np.array_equal(state.to_host(), np.abs(host).max(axis=axis).view(np.uint32)):
            raise AssertionError(f"nqk_absmax_f32 differs from np.abs(x).max({axis}) on [{rows}, {cols}]")
        del host

        def absmax():
            for _ in range(args.reps):
                for s in srcs:
                    _lib.call("nqk_absmax_f32", s.vp, rows, cols, cols, axis, state.vp)

        def hist():
            for _ in range(args.reps):
                for s in srcs:
                    _lib.call("nqk_hist_f32", s.vp, s.size, hstate.vp, 0)

        def copy():
            for _ in range(args.reps):
                for s in srcs:
                    _lib.call("nqk_memcpy_d2d", dst.vp, s.vp, nbytes)

        legs = {"absmax": absmax, "hist_range": hist, "copy_d2d": copy}
        samples = {k: [] for k in legs}
        for i in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                ms = _timer_ms(fn)
                if i >= args.warmup:
                    samples[name].append(1e3 * ms / (args.reps * copies))
        sync()
        tag = f"{rows}x{cols}_axis{axis}"
        res[f"{tag}_bytes"], res[f"{tag}_buffers"] = nbytes, copies
        for name, smp in samples.items():
            us, mm = _stats(smp, 2)
            res[f"{tag}_{name}_us"], res[f"{tag}_{name}_us_min_max"] = us, mm
            moved = nbytes * (2 if name == "copy_d2d" else 1)  # a copy reads and writes every byte
            res[f"{tag}_{name}_TBps"] = round(moved / (us * 1e-6) / 1e12, 3)
            if name != "copy_d2d":
                res[f"{tag}_{name}_fraction_of_copy_rate"] = round(nbytes / (us * 1e-6) / COPY_RATE, 3)
        res[f"{tag}_absmax_over_hist_range"] = round(res[f"{tag}_absmax_us"] / res[f"{tag}_hist_range_us"], 3)
        del srcs, dst
    return res


def step_cost(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.device import sync
    from numpy_quant.model import Model
    _lib.ensure_init()
    calib = args.calib
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    model.rebatch(calib)
    x = np.random.default_rng(12345).standard_normal((calib, 3, 224, 224)).astype(np.float32)

    def forward_only():
        model._forward([x])
        sync()

    def equalize():
        model.equalize([[x]])
        sync()

    legs = {"equalize": equalize, "calibrate_stream": lambda: model.calibrate_stream([[x]]), "forward_only": forward_only}
    samples = {k: [] for k in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0))
    eqm = model.equalize([[x]])
    res = {"cost_calibration_images": calib, "cost_sites": len(eqm.equalization.sites),
           "cost_nonzero_exponents": int(sum(np.count_nonzero(s.vector) for s in eqm.equalization.sites))}
    for name, smp in samples.items():
        res[f"cost_{name}_ms"], res[f"cost_{name}_ms_min_max"] = _stats(smp, 2)
    return res


CONFIGS = (("w8a8", dict(bit_width=8)), ("w8a8_per_column", dict(bit_width=8, per_channel=True)),
           ("w4a8_per_column", dict(bit_width=8, weight_bit_width=4, per_channel=True)), ("w4a4", dict(bit_width=4)))


def step_error(args) -> dict:
    from numpy_quant.model import Model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _equalize_ref as R
    res = {}
    for fixture, outliers in (("outliers", True), ("plain_weights", False)):
        proto, _, x, _ = R.outlier_fixture(MODELS, outliers=outliers)
        model = Model.from_onnx(proto)
        out = model.outputs[0].name
        legs = [("plain", model)]
        for alpha in ((0.25, 0.5, 0.75) if outliers else (0.5,)):
            legs.append((f"alpha{alpha}", model.equalize([[x]], alpha=alpha)))
        ref = model([x])[0]
        for tag, m in legs:
            if not np.array_equal(m([x])[0].view(np.uint32), ref.view(np.uint32)):
                raise AssertionError(f"the equalized float model ({tag}) is not bit-identical to the source")
            if m.equalization is not None:
                e = np.concatenate([s.vector for s in m.equalization.sites])
                res[f"error_{fixture}_{tag}_exponent_min_max"] = [int(e.min()), int(e.max())]
                res[f"error_{fixture}_{tag}_exponents_nonzero"] = int(np.count_nonzero(e))
            sites = (m.equalization or model.equalize([[x]]).equalization).sites
            for cfg, kw in CONFIGS:
                rep = m.compare(m.quantize([x], **kw), [[x]], k=1)
                key = f"error_{fixture}_{cfg}_{tag}"
                res[f"{key}_output_mse"] = float(rep.values[out].mse)
                res[f"{key}_output_sqnr_db"] = round(float(rep.values[out].sqnr_db), 3)
                res[f"{key}_ln_output_sqnr_db"] = [round(float(rep.values[s.out].sqnr_db), 2) for s in sites]
                wq = [float(rep.values[w].sqnr_db) for s in sites for w in s.weights]
                res[f"{key}_site_weight_sqnr_db_min_max"] = [round(min(wq), 2), round(max(wq), 2)]
    return res


def step_step(args) -> dict:
    from numpy_quant import kernels as K
    from numpy_quant import onnx_proto
    from numpy_quant.model import Model
    from numpy_quant.tensor import FTensor
    B = args.step_batch
    x_cal = np.random.default_rng(12345).standard_normal((8, 3, 224, 224)).astype(np.float32)
    x_dev = FTensor(np.random.default_rng(256).standard_normal((B, 3, 224, 224)).astype(np.float32))
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    model.rebatch(8)
    eqm = model.equalize([[x_cal]])
    qs = {"plain": model.quantize([x_cal], bit_width=8), "equalized": eqm.quantize([x_cal], bit_width=8)}
    res = {"step_batch": B, "step_sites": len(eqm.equalization.sites),
           "step_nonzero_exponents": int(sum(np.count_nonzero(s.vector) for s in eqm.equalization.sites))}
    for m in (model, eqm):
        for v in m.values:  # free the float calibration activations
            if v.__class__.__name__ == "Variable":
                v.data = None
    model.rebatch(B)  # the node attributes are shared: both QModels follow
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
            us = sorted(1e3 * ms for t, ms, _, _ in recs if t == tag)
            res[f"step_{name}_{tag}_us"] = round(statistics.median(us), 1)
            res[f"step_{name}_{tag}_launches"] = len(us)
        graphs[name] = q.graph([x_dev])
        if not np.array_equal(graphs[name].run_device([x_dev])[0].dev.to_host(), logits[name]):
            raise AssertionError(f"graph replay differs from the plain call ({name})")
    samples = {k: [] for k in graphs}
    for i in range(args.warmup + args.rounds):
        for name, g in graphs.items():
            ms = _timer_ms(lambda: [g.run_device([x_dev]) for _ in range(args.steps)])
            if i >= args.warmup:
                samples[name].append(ms / args.steps)
    res["step_fused_layers"] = {k: q._plan.fused for k, q in qs.items()}
    res["step_cls_tails"] = {k: q._plan.cls_tails for k, q in qs.items()}
    for name, smp in samples.items():
        res[f"step_{name}_ms"], res[f"step_{name}_ms_min_max"] = _stats(smp)
    res["step_top1_agreement_equalized_vs_plain"] = float(np.mean(logits["equalized"].argmax(1) == logits["plain"].argmax(1)))
    for g in graphs.values():
        g.destroy()
    return res


STEPS = {"kernel": (step_kernel, 180), "cost": (step_cost, 180), "error": (step_error, 240), "step": (step_step, 420)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calib", type=int, default=8, help="calibration images of the cost step")
    ap.add_argument("--step-batch", type=int, default=256, help="images of the graph-replayed forward")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="passes over the buffers per timed window")
    ap.add_argument("--steps", type=int, default=5, help="graph replays per timed window")
    ap.add_argument("--only", help="comma-separated steps to run (default: all)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "channel equalization (Model.equalize): kernel, cost, error and step", "rounds": args.rounds}
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}"
                   for k in ("calib", "step_batch", "rounds", "warmup", "reps", "steps")]
    only = set(args.only.split(",")) if args.only else set(STEPS)
    for name, (_, limit) in STEPS.items():
        if name not in only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_equalize] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_equalize] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
