#!/usr/bin/env python
"""Streamed calibration on one MI355X.  Prints one JSON line.

  micro   nqk_hist_f32 alone, with the library's stream timer (device events): float32
          [50432, 768] and [50432, 3072] of standard-normal data and the same after a ReLU (half
          the elements exact zeros), rotating over more than 256 MiB of buffers, with counts and
          with the range only, as bytes over time beside the device copy rate; and both of its
          kernels (straight global atomics / per-workgroup LDS histograms, forced with
          NQK_HIST_DIRECT_MAX) at 1 Ki .. 1 Mi elements, which is what HIST_DIRECT_MAX is set from
  e2e     Model.calibrate against Model.calibrate_stream on the bench's ViT-Base calibration
          (8 images, seed 12345, synthetic weights) at percentile 100 and 99.99

The kernel's state is compared with np.bincount, and calibrate_stream at 100 with calibrate (every
value, by equality), before anything is reported.  The legs of `e2e` are timed in alternating
rounds in one process; the figure of a leg is the median of its rounds.  Each GPU step is a child
process under its own time limit; after a step that fails or runs out of time nothing more is
started.
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
SMALL = [1 << 10, 1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16, 1 << 18, 1 << 20]


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


def step_micro(args) -> dict:
    from numpy_quant import _lib
    from numpy_quant import calibration as C
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray, sync
    _lib.ensure_init()
    rng = np.random.default_rng(2027)
    res = {"hist_direct_max": K.HIST_DIRECT_MAX}
    fresh = C.fresh_state()
    for cols in (768, 3072):
        nbytes = BIG_ROWS * cols * 4
        copies = max(1, -(-(320 << 20) // nbytes))  # more than 256 MiB in flight
        for kind in ("normal", "relu"):
            hosts = [rng.standard_normal((BIG_ROWS, cols), dtype=np.float32) for _ in range(copies)]
            if kind == "relu":
                hosts = [np.maximum(h, np.float32(0)) for h in hosts]
            srcs = [DeviceArray.from_host(h) for h in hosts]
            state = DeviceArray.from_host(fresh)
            _lib.call("nqk_hist_f32", srcs[0].vp, srcs[0].size, state.vp, 1)
            if not np.array_equal(state.to_host(), C.host_state(hosts[0])):
                raise AssertionError(f"nqk_hist_f32 differs from np.bincount on {kind} [{BIG_ROWS}, {cols}]")
            del hosts
            for counts in (1, 0):
                def rounds():
                    for _ in range(args.reps):
                        for s in srcs:
                            _lib.call("nqk_hist_f32", s.vp, s.size, state.vp, counts)
                us, lo, hi = _median_us(rounds, args.reps * copies, args)
                tag = f"hist_{kind}_{cols}_{'counts' if counts else 'range'}"
                res[f"{tag}_us"] = round(us, 2)
                res[f"{tag}_us_min_max"] = [round(lo, 2), round(hi, 2)]
                res[f"{tag}_TBps"] = round(nbytes / (us * 1e-6) / 1e12, 3)
                res[f"{tag}_fraction_of_copy_rate"] = round(nbytes / (us * 1e-6) / COPY_RATE, 3)
            res[f"hist_{cols}_bytes"] = nbytes
            res[f"hist_{cols}_buffers"] = copies
            sync()
            del srcs
    # the two kernels at one size: NQK_HIST_DIRECT_MAX is read on every call
    pool = DeviceArray.from_host(rng.standard_normal(SMALL[-1] * 8, dtype=np.float32))
    state = DeviceArray.from_host(fresh)
    try:
        for n in SMALL:
            views = [pool.offset_view(k * n, (n,)) for k in range(8)]
            for kind, env in (("direct", str(1 << 40)), ("lds", "0")):
                os.environ["NQK_HIST_DIRECT_MAX"] = env
                _lib.call("nqk_memcpy_h2d", state.vp, ctypes.c_void_p(fresh.ctypes.data), fresh.nbytes)
                _lib.call("nqk_hist_f32", views[0].vp, n, state.vp, 1)
                if not np.array_equal(state.to_host(), C.host_state(pool.offset_view(0, (n,)).to_host())):
                    raise AssertionError(f"nqk_hist_f32 ({kind}) differs from np.bincount at n = {n}")

                def rounds():
                    for _ in range(args.small_reps):
                        for v in views:
                            _lib.call("nqk_hist_f32", v.vp, n, state.vp, 1)
                us, lo, hi = _median_us(rounds, args.small_reps * len(views), args)
                res[f"hist_{kind}_n{n}_us"] = round(us, 2)
                res[f"hist_{kind}_n{n}_us_min_max"] = [round(lo, 2), round(hi, 2)]
    finally:
        os.environ.pop("NQK_HIST_DIRECT_MAX", None)
    sync()
    return res


def step_e2e(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.calibration import STATE_LEN, Calibrator
    from numpy_quant.device import sync
    from numpy_quant.model import Model
    from numpy_quant.tensor import FTensor
    _lib.ensure_init()
    calib = args.calib
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    model.rebatch(calib)
    x = np.random.default_rng(12345).standard_normal((calib, 3, 224, 224)).astype(np.float32)

    want = model.calibrate([x])
    got = model.calibrate_stream([[x]])
    for w, g in zip(want, got):
        if set(w) != set(g) or any(not (w[k] == g[k]) for k in w):
            raise AssertionError("calibrate_stream at percentile 100 differs from calibrate")
    clipped = model.calibrate_stream([[x]], percentile=99.99)
    narrower = sum(1 for k in want[1] if clipped[1][k] < want[1][k] or clipped[0][k] > want[0][k])

    def forward_only():
        model._forward([x])
        sync()

    legs = {"calibrate": lambda: model.calibrate([x]),
            "stream_100": lambda: model.calibrate_stream([[x]]),
            "stream_99_99": lambda: model.calibrate_stream([[x]], percentile=99.99),
            "forward_only": forward_only}
    samples = {name: [] for name in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():  # alternating: the same box, the same minutes
            t0 = time.perf_counter()
            fn()  # every leg ends in a synchronous read-back or a sync
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0))
    # the parts of a streamed calibration after its forward: the observe loop (one kernel per
    # device value) up to the device's last kernel, and ranges() (download + host arithmetic)
    parts = {}
    for tag, pct in (("100", 100.0), ("99_99", 99.99)):
        obs, rng_ms = [], []
        for i in range(args.warmup + args.rounds):
            cal = Calibrator(pct)
            forward_only()
            t0 = time.perf_counter()
            cal.observe(model)
            sync()
            t1 = time.perf_counter()
            cal.ranges()
            t2 = time.perf_counter()
            if i >= args.warmup:
                obs.append(1e3 * (t1 - t0))
                rng_ms.append(1e3 * (t2 - t1))
        parts[f"observe_{tag}_ms"] = round(statistics.median(obs), 2)
        parts[f"ranges_{tag}_ms"] = round(statistics.median(rng_ms), 2)
    n_dev = sum(1 for v in model.values if isinstance(v.data, FTensor))
    elements = sum(v.data.dev.size for v in model.values if isinstance(v.data, FTensor))
    res = {"calib_images": calib, "values": len(model.values), "device_values": n_dev,
           "device_value_elements": int(elements), "arena_bytes": n_dev * STATE_LEN * 8,
           "values_verified_equal_at_100": len(want[0]), "values_narrower_at_99_99": narrower, **parts}
    for name, s in samples.items():
        res[f"{name}_ms"] = round(statistics.median(s), 2)
        res[f"{name}_ms_min_max"] = [round(min(s), 2), round(max(s), 2)]
    return res


STEPS = {"micro": (step_micro, 300), "e2e": (step_e2e, 420)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calib", type=int, default=8, help="calibration images")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="launches per large buffer and timed window")
    ap.add_argument("--small-reps", dest="small_reps", type=int, default=50,
                    help="launches per small buffer and timed window")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "streamed calibration: nqk_hist_f32 alone, and Model.calibrate against calibrate_stream "
                        "on ViT-Base (synthetic weights, seed 12345)",
              "rounds": args.rounds,
              "verified": "nqk_hist_f32 equals np.bincount and the exact key range; calibrate_stream at "
                          "percentile 100 equals calibrate on every value"}
    passthrough = [f"--{name.replace('_', '-')}={getattr(args, name)}"
                   for name in ("calib", "rounds", "warmup", "reps", "small_reps")]
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_calibration] step {name} ran past its {limit} s limit; nothing more is started",
                  file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_calibration] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
            return p.returncode or 1
        result.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
