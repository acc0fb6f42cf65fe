#!/usr/bin/env python
"""The Conv in integers (QModel.integer_conv) against the reference-exact float Conv, at the
headline shape (ViT-Base int8, B = 256, synthetic weights), on one MI355X.  Prints one JSON line
(and writes it to --out).

  kernel  nqk_embed_q (f32 MFMA, OpenBLAS summation order) against nqk_embed_qi8 (int8 MFMA) at
          [B, 3, 224, 224] -> 768 and -> 192, library stream timer, rotating over two buffer sets
          (more than the 256 MiB Infinity Cache together): us and fraction of the copy rate
  step    the graph-replayed B = 256 ViT-Base int8 forward with the flag off and on
  error   model.compare of both QModels against the float model on the 8 calibration images:
          the embedding output's mean |d| and SQNR, the logits' top-1 agreement

The legs of a step alternate in one process; a figure is the median of its --rounds windows,
with min-max.  The integer kernel's output is compared with a NumPy restatement (first and last
images) before anything is timed.  Each GPU step is a child process under its own time limit;
after a step that fails or runs out of time nothing more is started.
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

COPY_RATE = 6.29e12  # B/s, the device copy rate DESIGN.md quotes
MODEL_FILE = os.path.join(ROOT, "numpy-quant_amd", "models", "vit_image_classifier_no_weights.onnx")


def _timer_ms(fn) -> float:
    from numpy_quant import _lib
    _lib.call("nqk_timer_start")
    fn()
    _lib.call("nqk_timer_stop")
    ms = ctypes.c_float()
    _lib.call("nqk_timer_ms", ctypes.byref(ms))
    return ms.value


def _stats(samples, digits=2):
    return round(statistics.median(samples), digits), [round(min(samples), digits), round(max(samples), digits)]


def _restate_embed(xq, zx, sx, wq, sw, bias, cls, pos):
    """The integer embedding of a few images in NumPy: float64 products of these integers are exact."""
    n, c, h, w = xq.shape
    kout = wq.shape[0]
    ho, wo = h // 16, w // 16
    cols = xq.reshape(n, c, ho, 16, wo, 16).transpose(0, 2, 4, 1, 3, 5).reshape(n * ho * wo, c * 256)  # (ci, ki, kj)
    wm = wq.reshape(kout, c * 256)
    acc = np.rint(cols.astype(np.float64) @ wm.T.astype(np.float64)).astype(np.int64)
    v = acc - np.int64(zx) * wm.sum(1, dtype=np.int64)[None, :]
    y = (v.astype(np.float64) * np.float64(np.float32(sx * sw))).astype(np.float32).reshape(n, ho * wo, kout)
    out = np.empty((n, ho * wo + 1, kout), np.float32)
    out[:, 0] = cls + pos[0]
    out[:, 1:] = (y + bias) + pos[1:]
    return out


def step_kernel(args) -> dict:
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray, sync
    from numpy_quant.plan import embed_weight_image
    _lib.ensure_init()
    B, c, h, w = args.batch, 3, 224, 224
    hw, kk = (h // 16) * (w // 16), c * 256
    rng = np.random.default_rng(7)
    zx, sx, sw = -3, np.float32(0.0187), np.float32(0.0021)
    xq = rng.integers(-128, 128, size=(B, c, h, w), dtype=np.int8)
    sets = 2  # 2 x (38.5 MB image + 154 MB output at N = 768) > 256 MiB
    qs = [DeviceArray.from_host(xq) for _ in range(sets)]
    res = {}
    for n_out in (768, 192):
        wq = rng.integers(-127, 128, size=(n_out, c, 16, 16), dtype=np.int8)
        bias = rng.standard_normal(n_out).astype(np.float32)
        cls = rng.standard_normal(n_out).astype(np.float32)
        pos = rng.standard_normal((hw + 1, n_out)).astype(np.float32)
        wm = wq.reshape(n_out, kk).astype(np.int64)
        d_wq = DeviceArray.from_host(wq.reshape(n_out, kk))
        d_ct = DeviceArray.from_host((wm.sum(1) * zx).astype(np.int32))
        l1 = int(np.abs(wm).sum(1).max())
        wf = (wq.astype(np.float64) * np.float64(sw)).astype(np.float32)  # the dequantized weight of the float path
        d_wt = embed_weight_image(DeviceArray.from_host(wf), n_out, kk)
        d_bias, d_cls, d_pos = (DeviceArray.from_host(a) for a in (bias, cls, pos))
        outs = [DeviceArray((B, hw + 1, n_out), np.float32) for _ in range(sets)]
        scale = np.float32(sx * sw)

        def run_f32():
            for q, o in zip(qs, outs):
                _lib.call("nqk_embed_q", q.vp, float(sx), zx, d_wt.vp, d_bias.vp, d_cls.vp, d_pos.vp, o.vp, B, c, h, w,
                          16, 16, n_out)

        def run_qi8():  # the bare entry point, as the f32 leg (kernels.embed_qi8's host checks ran once below)
            for q, o in zip(qs, outs):
                _lib.call("nqk_embed_qi8", q.vp, d_wq.vp, d_ct.vp, float(scale), zx, l1, d_bias.vp, d_cls.vp, d_pos.vp,
                          o.vp, B, c, h, w, 16, 16, n_out)

        for q, o in zip(qs, outs):
            K.embed_qi8(q, d_wq, d_ct, scale, zx, l1, d_bias, d_cls, d_pos, o)
        sync()
        for o in outs:
            got = o.to_host()
            for sl in (slice(0, 2), slice(B - 2, B)):
                want = _restate_embed(xq[sl].astype(np.int64), zx, sx, wq.astype(np.int64), sw, bias, cls, pos)
                if not np.array_equal(got[sl], want):
                    raise AssertionError(f"nqk_embed_qi8 differs from the NumPy restatement (N = {n_out})")
        legs = {"embed_q": run_f32, "embed_qi8": run_qi8}
        samples = {k: [] for k in legs}
        for i in range(args.warmup + args.rounds):
            for name, fn in legs.items():  # alternating: the same box, the same minutes
                ms = _timer_ms(lambda: [fn() for _ in range(args.reps)])
                if i >= args.warmup:
                    samples[name].append(1e3 * ms / (args.reps * sets))
        moved = {"embed_q": B * c * h * w + 4 * kk * n_out + 4 * B * (hw + 1) * n_out,
                 "embed_qi8": B * c * h * w + kk * n_out + 4 * B * (hw + 1) * n_out}
        for name, s in samples.items():
            us, mm = _stats(s)
            res[f"{name}_n{n_out}_us"] = us
            res[f"{name}_n{n_out}_us_min_max"] = mm
            res[f"{name}_n{n_out}_fraction_of_copy_rate"] = round(moved[name] / (us * 1e-6) / COPY_RATE, 3)
        res[f"embed_qi8_n{n_out}_int8_TOPS"] = round(2 * B * hw * kk * n_out / (res[f"embed_qi8_n{n_out}_us"] * 1e-6) / 1e12, 1)
        res[f"ranges_overlap_n{n_out}"] = bool(max(samples["embed_qi8"]) >= min(samples["embed_q"]))
    res["kernel_buffer_sets"] = sets
    sync()
    return res


def _build(batch_cal=8):
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.model import Model
    _lib.ensure_init()
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    model.rebatch(batch_cal)
    x_cal = np.random.default_rng(12345).standard_normal((batch_cal, 3, 224, 224)).astype(np.float32)  # bench.py's
    qoff = model.quantize([x_cal], bit_width=8)
    qon = model.quantize_with(qoff.quant_params, bit_width=8, integer_conv=True)
    return model, qoff, qon, x_cal


def step_step(args) -> dict:
    from numpy_quant.tensor import FTensor
    model, qoff, qon, _ = _build()
    for v in model.values:  # free the float calibration activations
        if v.__class__.__name__ == "Variable":
            v.data = None
    B = args.batch
    model.rebatch(B)  # shared attribute dicts: rebatches the QModels too
    x_dev = FTensor(np.random.default_rng(256).standard_normal((B, 3, 224, 224)).astype(np.float32))
    logits, graphs = {}, {}
    for name, q in (("off", qoff), ("on", qon)):
        logits[name] = q([x_dev])[0]
        graphs[name] = q.graph([x_dev])
        if not np.array_equal(graphs[name].run_device([x_dev])[0].dev.to_host(), logits[name]):
            raise AssertionError(f"graph replay differs from the plain call (integer_conv {name})")
    samples = {k: [] for k in graphs}
    for i in range(args.warmup + args.rounds):
        for name, g in graphs.items():
            ms = _timer_ms(lambda: [g.run_device([x_dev]) for _ in range(args.steps)])
            if i >= args.warmup:
                samples[name].append(ms / args.steps)
    res = {"step_fused_layers": qon._plan.fused, "step_embeds": qon._plan.embeds, "steps_per_window": args.steps}
    for name, s in samples.items():
        ms, mm = _stats(s, 3)
        res[f"step_{name}_ms"] = ms
        res[f"step_{name}_ms_min_max"] = mm
        res[f"step_{name}_images_per_s"] = round(B / (ms * 1e-3), 1)
    res["step_ranges_overlap"] = bool(max(samples["on"]) >= min(samples["off"]))
    res["step_top1_agreement_on_vs_off"] = float(np.mean(logits["on"].argmax(1) == logits["off"].argmax(1)))
    for g in graphs.values():
        g.destroy()
    return res


def step_error(args) -> dict:
    model, qoff, qon, x_cal = _build()
    plan = qon.compile()
    emb = next(s.m.add.outputs[0].name for k, s in plan.steps if k == "embed")
    res = {"error_rows": int(x_cal.shape[0]), "embedding_value": emb}
    for name, q in (("off", qoff), ("on", qon)):
        rep = model.compare(q, [[x_cal]], k=5, values=True)
        s = rep.values[emb]
        res[f"error_{name}_embedding_mean_abs"] = float(s.mean_abs)
        res[f"error_{name}_embedding_sqnr_db"] = round(float(s.sqnr_db), 3)
        res[f"error_{name}_top1_agreement"] = float(rep.top1_agreement)
    return res


STEPS = {"kernel": (step_kernel, 300), "step": (step_step, 540), "error": (step_error, 300)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="kernel launches per buffer set and timed window")
    ap.add_argument("--steps", type=int, default=30, help="graph replays per timed window")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    result = {"metric": "Conv in integers (QModel.integer_conv) against the float Conv, ViT-Base int8 (synthetic weights)",
              "batch": args.batch, "rounds": args.rounds,
              "verified": "nqk_embed_qi8 equals the NumPy restatement on the first and last images; each graph "
                          "replay equals its plain call"}
    passthrough = [f"--{k}={getattr(args, k)}" for k in ("batch", "rounds", "warmup", "reps", "steps")]
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_conv] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_conv] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
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
