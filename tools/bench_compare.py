#!/usr/bin/env python
"""The quantization error report on one MI355X.  Prints one JSON line.

  micro   nqk_compare_stats alone (both of its launches), with the library's stream timer (device
          events): float32 x of [50432, 768] and [50432, 3072] against y as float32, int8 and int64
          storage, rotating over more than 256 MiB of buffers, as bytes read over time beside the
          device copy rate; beside it on the same x the two yardsticks, nqk_hist_f32's range-only
          pass and nqk_minmax_f32
  e2e     ViT-Base, 8 images (seed 12345, synthetic weights), int8: model.compare(qmodel, [batch])
          against the host route (both forwards, then every value of both models downloaded and
          the same statistics in NumPy), and the two forwards alone

The kernel's state is compared with compare.host_state, and the report with the host route's
numbers, before anything is reported.  The legs of `e2e` are timed in alternating rounds in one
process; the figure of a leg is the median of its rounds.  Each GPU step is a child process under
its own time limit; after a step that fails or runs out of time nothing more is started.
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
BIG_ROWS = 50432     # 256 images x 197 tokens


def _timer_ms(fn) -> float:
    from numpy_quant import _lib
    _lib.call("nqk_timer_start")
    fn()
    _lib.call("nqk_timer_stop")
    ms = ctypes.c_float()
    _lib.call("nqk_timer_ms", ctypes.byref(ms))
    return ms.value


def _median_us(fn, launches, args):
    samples = []
    for i in range(args.warmup + args.rounds):
        ms = _timer_ms(fn)
        if i >= args.warmup:
            samples.append(1e3 * ms / launches)
    return statistics.median(samples), min(samples), max(samples)


def _rate(res, tag, nbytes, timing):
    us, lo, hi = timing
    res[f"{tag}_us"] = round(us, 2)
    res[f"{tag}_us_min_max"] = [round(lo, 2), round(hi, 2)]
    res[f"{tag}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
    res[f"{tag}_fraction_of_copy_rate"] = round(nbytes / (us * 1e-6) / COPY_RATE, 3)


def step_micro(args) -> dict:
    from numpy_quant import _lib
    from numpy_quant import compare as C
    from numpy_quant import kernels as K
    from numpy_quant.calibration import fresh_state
    from numpy_quant.device import DeviceArray, sync
    _lib.ensure_init()
    rng = np.random.default_rng(2028)
    res = {}
    scale, zp = np.float32(0.03), 3
    for cols in (768, 3072):
        n = BIG_ROWS * cols
        chunks = -(-n // K.CMP_CHUNK)
        scratch = DeviceArray((3 * chunks,), np.float64)
        state = DeviceArray((K.CMP_STATE,), np.int64).fill_zero()
        for kind, ydt in (("f32", np.float32), ("i8", np.int8), ("i64", np.int64)):
            pair_bytes = n * (4 + np.dtype(ydt).itemsize)
            copies = max(1, -(-(320 << 20) // pair_bytes))  # more than 256 MiB between two reads of a line
            xs, ys = [], []
            for c in range(copies):
                x = rng.standard_normal((BIG_ROWS, cols), dtype=np.float32)
                q = np.clip(np.rint(x / scale) + zp, -128, 127)
                y = ((q - zp) * scale).astype(np.float32) if ydt == np.float32 else q.astype(ydt)
                if c == 0 and cols == 768:  # the state against the NumPy statement, once per kind
                    yf = y if ydt == np.float32 else ((q - zp).astype(np.float64) * np.float64(scale)).astype(np.float32)
                    want = C.host_state(x, yf)
                xs.append(DeviceArray.from_host(x))
                ys.append(DeviceArray.from_host(y))
                del x, q, y
            code = _lib.NQK_F32 if ydt == np.float32 else ys[0].code

            def call(k):
                _lib.call("nqk_compare_stats", xs[k].vp, ys[k].vp, code, float(scale), zp, 1, n, state.vp, scratch.vp,
                          3 * chunks)
            if cols == 768:
                state.fill_zero()
                call(0)
                if not np.array_equal(state.to_host(), want):
                    raise AssertionError(f"nqk_compare_stats differs from compare.host_state on {kind} [{BIG_ROWS}, {cols}]")

            def rounds():
                for _ in range(args.reps):
                    for k in range(copies):
                        call(k)
            tag = f"compare_{kind}_{cols}"
            _rate(res, tag, pair_bytes, _median_us(rounds, args.reps * copies, args))
            res[f"{tag}_bytes"] = pair_bytes
            res[f"{tag}_buffers"] = copies
            if kind == "f32":  # the yardsticks on the same x (and y, to rotate over as many bytes)
                hstate = DeviceArray.from_host(fresh_state())
                mm, mscratch = DeviceArray((2,), np.float32), DeviceArray((4096,), np.float32)
                both = xs + ys

                def hist():
                    for _ in range(args.reps):
                        for s in both:
                            _lib.call("nqk_hist_f32", s.vp, n, hstate.vp, 0)

                def minmax():
                    for _ in range(args.reps):
                        for s in both:
                            _lib.call("nqk_minmax_f32", s.vp, n, mm.vp, mscratch.vp, 4096)
                _rate(res, f"hist_range_{cols}", 4 * n, _median_us(hist, args.reps * len(both), args))
                _rate(res, f"minmax_{cols}", 4 * n, _median_us(minmax, args.reps * len(both), args))
            sync()
            del xs, ys
    return res


def _host_stats(x, y):
    """the report's figures of one value, plainly in NumPy float64 (np.sum's order)"""
    x, y = x.ravel(), y.ravel()
    ok = np.isfinite(x) & np.isfinite(y)
    xd = x[ok].astype(np.float64)
    d = xd - y[ok].astype(np.float64)
    return int(ok.sum()), float(np.abs(d).sum()), float((d * d).sum()), float((xd * xd).sum()), float(np.abs(d).max())


def step_e2e(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.device import sync
    from numpy_quant.model import Constant, Model
    from numpy_quant.tensor import FTensor, QTensor
    _lib.ensure_init()
    images = args.images
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    model.rebatch(images)
    x = np.random.default_rng(12345).standard_normal((images, 3, 224, 224)).astype(np.float32)
    qmodel = model.quantize([x], bit_width=8)

    def forwards():
        model._forward([x])
        kept = {v.name: v.data for v in model.inputs}
        qmodel.set_inputs([x])
        qmodel.run(eager=True)
        return kept

    def forwards_only():
        forwards()
        sync()

    def host_route():
        kept = forwards()
        theirs = {v.name: v for v in qmodel.values}
        out = {}
        for v in model.values:
            ref = kept.get(v.name, v.data)
            q = theirs.get(v.name)
            if q is None or not isinstance(ref, FTensor):
                continue
            got = q.data.dequantize().data if isinstance(q.data, QTensor) else q.data.data
            out[v.name] = _host_stats(ref.data, got)
        return out

    def device_route():
        return model.compare(qmodel, [[x]], k=5)

    rep, host = device_route(), host_route()
    if set(rep.values) != set(host):
        raise AssertionError("the two routes cover different values")
    for name, (count, sa, sd, sx, mx) in host.items():
        s = rep.values[name]
        f = rep.states[name].view(np.float64)
        tol = max(count - 1, 1) * 2.0 ** -52  # each order lies within (n - 1) 2^-53 of the exact sum
        if s.count != count or s.max_abs != mx or any(abs(a - b) > tol * abs(b) for a, b in zip(f[2:5], (sa, sd, sx))):
            raise AssertionError(f"{name}: the report differs from the host route")
    legs = {"compare": device_route, "forwards_only": forwards_only, "host_route": host_route}
    samples = {name: [] for name in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():  # alternating: the same box, the same minutes
            t0 = time.perf_counter()
            fn()  # every leg ends in a synchronous read-back or a sync
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0))
        # the host route dequantizes every quantized value into a new buffer, which leaves the
        # caching allocator with blocks of other sizes than the forwards ask for; the forwards
        # that follow pay hipMalloc for theirs (measured: 440 ms instead of 40).  A loop over
        # evaluation batches never sees that, so one untimed pass restores its steady state.
        forwards_only()
    elements = sum(int(s.count + s.nonfinite) for s in rep.values.values())
    out = model.outputs[0].name
    res = {"images": images, "values_compared": len(rep.values),
           "constants_compared": sum(1 for v in model.values if isinstance(v, Constant) and v.name in rep.values),
           "elements_compared": elements, "host_route_download_bytes": 8 * elements,
           "values_verified_against_host_route": len(host),
           "output_mean_abs": rep.values[out].mean_abs, "output_sqnr_db": rep.values[out].sqnr_db,
           "worst_sqnr_db": [[n, round(s.sqnr_db, 2)] for n, s in rep.worst(3)]}
    for name, s in samples.items():
        res[f"{name}_ms"] = round(statistics.median(s), 2)
        res[f"{name}_ms_min_max"] = [round(min(s), 2), round(max(s), 2)]
    res["forwards_share_of_compare"] = round(res["forwards_only_ms"] / res["compare_ms"], 3)
    return res


STEPS = {"micro": (step_micro, 420), "e2e": (step_e2e, 420)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=8, help="evaluation images of the e2e step")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="launches per buffer and timed window")
    ap.add_argument("--only", choices=sorted(STEPS), help="run this step alone")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "quantization error report: nqk_compare_stats alone, and Model.compare against the host "
                        "route on ViT-Base int8 (synthetic weights, seed 12345)",
              "rounds": args.rounds,
              "verified": "nqk_compare_stats equals compare.host_state bit for bit; the report equals the host "
                          "route's NumPy figures (counts and maxima exactly, sums within (n - 1) 2^-52)"}
    passthrough = [f"--{name}={getattr(args, name)}" for name in ("images", "rounds", "warmup", "reps")]
    for name, (_, limit) in STEPS.items():
        if args.only and name != args.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_compare] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_compare] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
            return p.returncode or 1
        result.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
