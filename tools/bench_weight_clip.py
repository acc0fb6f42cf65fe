#!/usr/bin/env python
"""The weight clipping search (Model.quantize(weight_clip="mse")) on one MI355X.  Prints one JSON
line (and writes it to --out, e.g. profiles/weight_clip.json).

  kernel  nqk_clip_search_cols alone, library stream timer, on float32 [768, 3072] and [3072, 768]
          at G = 64 candidates and 4 bits, err written: us, weights x candidates per second, and the
          VALU instructions per second that implies at the 21 per element and candidate the ISA
          holds (11 of them the IEEE divide); beside it the NumPy restatement
          (tests/_clip_ref.search_cols) on one host core, whose result the kernel's must equal in bits
  cost    ViT-Base (synthetic weights), 8 calibration images, (8, 4) per column: wall time of
          model.quantize with the search against the same call without it, alternating
  error   model.compare's output MSE / SQNR and the eligible weights' own SQNR at (8, 4) and (4, 4),
          per tensor and per column, without and with the search: the tests' encoder layer with
          columns spread over 2^-3..2^3 (tests/_perchannel_ref.encoder_layer_fixture), and the
          equalized outlier fixture (tests/_equalize_ref.outlier_fixture, Model.equalize)

A figure is the median of its --rounds windows, with min-max.  Each GPU step is a child process
under its own time limit; after a step that fails or runs out of time nothing more is started.
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
for p in (os.path.join(ROOT, "numpy-quant_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

MODELS = os.path.join(ROOT, "numpy-quant_amd", "models")
MODEL_FILE = os.path.join(MODELS, "vit_image_classifier_no_weights.onnx")
VALU_PER_EVAL, DIVIDE_PER_EVAL = 21, 11  # counted in the loop of k_clip_search's gfx950 ISA


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
    import _clip_ref as R
    import _perchannel_ref as P
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray, sync
    _lib.ensure_init()
    rng = np.random.default_rng(2029)
    G, bw = 64, 4
    ratio = K.clip_ratios(G)
    res = {"kernel_candidates": G, "kernel_bit_width": bw, "kernel_valu_per_element_and_candidate": VALU_PER_EVAL,
           "kernel_divide_valu_per_element_and_candidate": DIVIDE_PER_EVAL}
    for rows, cols in ((768, 3072), (3072, 768)):
        host = (rng.standard_normal((rows, cols)) * np.exp2(rng.uniform(-3, 3, cols))).astype(np.float32)
        s0 = P.column_scales(host, 1, bw)
        w, s0d, rd = DeviceArray.from_host(host), DeviceArray.from_host(s0), DeviceArray.from_host(ratio)
        scale, index = DeviceArray((cols,), np.float32), DeviceArray((cols,), np.int32)
        err = DeviceArray((G, cols), np.float64)

        def search():
            for _ in range(args.reps):
                _lib.call("nqk_clip_search_cols", w.vp, rows, cols, cols, s0d.vp, rd.vp, G, bw, scale.vp, index.vp, err.vp)

        samples = []
        for i in range(args.warmup + args.rounds):
            ms = _timer_ms(search)
            if i >= args.warmup:
                samples.append(1e3 * ms / args.reps)
        sync()
        tag = f"kernel_{rows}x{cols}"
        us, mm = _stats(samples, 2)
        evals = rows * cols * G
        res[f"{tag}_us"], res[f"{tag}_us_min_max"] = us, mm
        res[f"{tag}_evaluations_per_s"] = round(evals / (us * 1e-6), -6)
        res[f"{tag}_valu_lane_instructions_per_s"] = round(evals * VALU_PER_EVAL / (us * 1e-6), -9)
        res[f"{tag}_bytes_read_per_s"] = round(rows * cols * 4 / (us * 1e-6), -6)
        res[f"{tag}_index_nonzero_fraction"] = round(float(np.mean(index.to_host() != 0)), 3)
        if rows == 768:  # the restatement once: a check in bits, and its time on one host core
            t0 = time.perf_counter()
            rs, ri, re = R.search_cols(host, s0, ratio, bw)
            res[f"{tag}_numpy_restatement_s"] = round(time.perf_counter() - t0, 2)
            if not (np.array_equal(scale.to_host().view(np.uint32), rs.view(np.uint32)) and np.array_equal(index.to_host(), ri)
                    and np.array_equal(err.to_host().view(np.uint64), re.view(np.uint64))):
                raise AssertionError(f"nqk_clip_search_cols differs from the restatement on [{rows}, {cols}]")
            res[f"{tag}_equals_restatement_in_bits"] = True
    return res


def step_cost(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.device import sync
    from numpy_quant.model import Model, per_channel_axis
    _lib.ensure_init()
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    model.rebatch(args.calib)
    x = np.random.default_rng(12345).standard_normal((args.calib, 3, 224, 224)).astype(np.float32)
    kw = dict(bit_width=8, weight_bit_width=4, per_channel=True)

    def leg(**extra):
        def run():
            model.quantize([x], **kw, **extra)
            sync()
        return run

    legs = {"quantize": leg(), "quantize_weight_clip": leg(weight_clip="mse")}
    samples = {k: [] for k in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0))
    weights = [v for v in model.values if per_channel_axis(v) is not None]
    res = {"cost_calibration_images": args.calib, "cost_config": "bit_width 8, weight_bit_width 4, per_channel",
           "cost_searched_weights": len(weights), "cost_searched_elements": int(sum(v.data.dev.size for v in weights))}
    for name, smp in samples.items():
        res[f"cost_{name}_ms"], res[f"cost_{name}_ms_min_max"] = _stats(smp, 1)
    return res


def step_error(args) -> dict:
    import _equalize_ref as E
    import _perchannel_ref as P
    from numpy_quant.model import Model, per_channel_axis
    res = {}
    spread = Model.from_onnx(P.encoder_layer_fixture(MODELS)[0]), P.encoder_layer_fixture(MODELS)[2]
    proto, _, xo, _ = E.outlier_fixture(MODELS)
    fixtures = {"spread_columns": spread, "equalized_outliers": (Model.from_onnx(proto).equalize([[xo]]), xo)}
    for fixture, (model, x) in fixtures.items():
        out = model.outputs[0].name
        weights = [v.name for v in model.values if per_channel_axis(v) is not None]
        for bw in (8, 4):
            for pc in (False, True):
                for clip in (None, "mse"):
                    q = model.quantize([x], bit_width=bw, weight_bit_width=4, per_channel=pc, weight_clip=clip)
                    rep = model.compare(q, [[x]], k=1)
                    key = f"error_{fixture}_a{bw}w4_{'per_column' if pc else 'per_tensor'}_{'search' if clip else 'plain'}"
                    wq = [float(rep.values[w].sqnr_db) for w in weights]
                    res[f"{key}_output_mse"] = float(rep.values[out].mse)
                    res[f"{key}_output_sqnr_db"] = round(float(rep.values[out].sqnr_db), 3)
                    res[f"{key}_weight_sqnr_db_min_max"] = [round(min(wq), 2), round(max(wq), 2)]
    return res


STEPS = {"kernel": (step_kernel, 240), "cost": (step_cost, 300), "error": (step_error, 300)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calib", type=int, default=8, help="calibration images of the cost step")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="kernel calls per timed window")
    ap.add_argument("--only", help="comma-separated steps to run (default: all)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "weight clipping search (weight_clip=\"mse\"): kernel, cost and error", "rounds": args.rounds}
    passthrough = [f"--{k}={getattr(args, k)}" for k in ("calib", "rounds", "warmup", "reps")]
    only = set(args.only.split(",")) if args.only else set(STEPS)
    for name, (_, limit) in STEPS.items():
        if name not in only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_weight_clip] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_weight_clip] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
