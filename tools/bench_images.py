#!/usr/bin/env python
"""uint8 image inputs at the headline shape (ViT-Base int8, B=256, synthetic weights), host
arrays in and logits out, on one MI355X.  Prints one JSON line.

  a  the float32 way: normalize on the host (ImagePreprocess.reference), qmodel([float32])
     (`a_float_only`: the same without the host normalize, the array already float32)
  b  qmodel([uint8]) with qmodel.image_preprocess set
  c  qmodel.classify_stream over several uint8 batches (pinned, double-buffered uploads)
and, with the library's stream timer: nqk_image_lut alone (rotating over buffer pairs larger
than the 256 MiB Infinity Cache together), the uint8 upload from pinned and from pageable
host memory.

With --resize, the same for decoded photos (B images of 375 x 500, shorter side to 256,
center crop 224: ImagePreprocess(resize=ResizeCrop(256, 224))): nqk_image_resize_lut alone, and
  r_list    qmodel([list of HWC uint8 images]), resize and crop on the device
  r_224     qmodel([uint8 224 x 224 batch]), the images already resized (leg b)
  r_pillow  the host recipe: Pillow resize + crop per image, then leg b (if Pillow imports)
  r_stream  qmodel.classify_stream over the lists

Every output row of b and c is compared with the float32 path's (bit for bit) before anything
is reported.  The legs a, b, c are timed in alternating rounds in one process; the figure of
a leg is the median of its rounds.  Each GPU step (micro, end to end) is a child process under
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

IMAGENET = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
COPY_RATE = 6.29e12  # B/s, the device copy rate DESIGN.md quotes
MODEL_FILE = os.path.join(ROOT, "numpy-quant_amd", "models", "vit_image_classifier_no_weights.onnx")


def _images(batch, count, seed=2024):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(batch, 224, 224, 3), dtype=np.uint8) for _ in range(count)]


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
    from numpy_quant.images import ImagePreprocess, PinnedBuffer
    _lib.ensure_init()
    pre = ImagePreprocess(*IMAGENET)
    B = args.batch
    shape = (B, 224, 224, 3)
    nbytes = int(np.prod(shape))
    pairs = max(1, -(-(320 << 20) // (2 * nbytes)))  # more than 256 MiB in flight
    imgs = _images(B, 1)[0]
    srcs = [DeviceArray.from_host(imgs) for _ in range(pairs)]
    lut, _ = K.quantize(pre.table_device(), 8, np.float32(0.02), -3)
    outs = [pre.lookup(s, shape, lut) for s in srcs]
    want = np.stack([lut.to_host()[c][imgs[..., c]] for c in range(3)], axis=1)
    for o in outs:
        if not np.array_equal(o.to_host(), want):
            raise AssertionError("nqk_image_lut differs from the NumPy gather")

    def lut_round():
        for s, o in zip(srcs, outs):
            _lib.call("nqk_image_lut", s.vp, lut.vp, lut.code, o.vp, B, 224, 224, 3, _lib.IMG_NHWC)

    samples = []
    for i in range(args.warmup + args.rounds):
        ms = _timer_ms(lambda: [lut_round() for _ in range(args.reps)])
        if i >= args.warmup:
            samples.append(1e3 * ms / (args.reps * pairs))
    lut_us = statistics.median(samples)
    res = {"lut_kernel_us": round(lut_us, 2), "lut_kernel_us_min_max": [round(min(samples), 2), round(max(samples), 2)],
           "lut_bytes": 2 * nbytes, "lut_buffer_pairs": pairs,
           "lut_TBps": round(2 * nbytes / (lut_us * 1e-6) / 1e12, 3),
           "lut_fraction_of_copy_rate": round(2 * nbytes / (lut_us * 1e-6) / COPY_RATE, 3)}

    pinned = PinnedBuffer(nbytes)
    np.copyto(pinned.array.reshape(shape), imgs)
    dst = srcs[0]
    for name, ptr in (("pinned", pinned.ptr), ("pageable", imgs.ctypes.data)):
        samples, wall = [], []
        for i in range(args.warmup + args.rounds):
            t0 = time.perf_counter()
            ms = _timer_ms(lambda: _lib.call("nqk_memcpy_h2d", dst.vp, ctypes.c_void_p(ptr), nbytes))
            wall.append(1e3 * (time.perf_counter() - t0))
            if i >= args.warmup:
                samples.append(ms)
        ms = statistics.median(samples)
        res[f"upload_{name}_ms"] = round(ms, 3)
        res[f"upload_{name}_ms_min_max"] = [round(min(samples), 3), round(max(samples), 3)]
        res[f"upload_{name}_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        res[f"upload_{name}_host_ms"] = round(statistics.median(wall[args.warmup:]), 3)
    res["upload_bytes"] = nbytes
    sync()
    pinned.free()
    return res


def step_e2e(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.images import ImagePreprocess
    from numpy_quant.model import Model
    _lib.ensure_init()
    pre = ImagePreprocess(*IMAGENET)
    B = args.batch
    batches = _images(B, args.stream_batches)
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    calib = min(8, B)
    model.rebatch(calib)
    qmodel = model.quantize([pre.reference(batches[0][:calib])], bit_width=8)
    for v in model.values:  # free the float calibration activations
        if v.__class__.__name__ == "Variable":
            v.data = None
    model.rebatch(B)
    qmodel.image_preprocess = pre
    plan = qmodel.compile()

    # every row of b and c against the float32 path
    want = [qmodel([pre.reference(b)])[0] for b in batches]
    for b, w in zip(batches, want):
        if not np.array_equal(qmodel([b])[0].view(np.uint32), w.view(np.uint32)):
            raise AssertionError("qmodel([uint8]) differs from the float32 path")
    for g, w in zip(qmodel.classify_stream(batches), want):
        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            raise AssertionError("classify_stream differs from the float32 path")

    x_f32 = pre.reference(batches[0])

    def leg_a():
        for b in batches:
            qmodel([pre.reference(b)])

    def leg_a_float_only():
        for _ in batches:
            qmodel([x_f32])

    def leg_b():
        for b in batches:
            qmodel([b])

    def leg_c():
        for _ in qmodel.classify_stream(batches):
            pass

    legs = {"a": leg_a, "a_float_only": leg_a_float_only, "b": leg_b, "c": leg_c}
    samples = {k: [] for k in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():  # alternating: the same box, the same minutes
            t0 = time.perf_counter()
            fn()  # every call ends in a synchronous read-back of the logits
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0) / len(batches))
    res = {"fused_layers": plan.fused, "rows_verified": int(sum(w.shape[0] for w in want)) * 2}
    for name, s in samples.items():
        res[f"{name}_ms_per_batch"] = round(statistics.median(s), 3)
        res[f"{name}_ms_min_max"] = [round(min(s), 3), round(max(s), 3)]
        res[f"{name}_images_per_s"] = round(B / (statistics.median(s) * 1e-3), 1)
    return res


SOURCE_HW = (375, 500)  # --resize: the decoded photo


def _photos(batch, count, seed=2025):
    rng = np.random.default_rng(seed)
    return [list(rng.integers(0, 256, size=(batch,) + SOURCE_HW + (3,), dtype=np.uint8)) for _ in range(count)]


def step_resize_micro(args) -> dict:
    from numpy_quant import _lib
    from numpy_quant import kernels as K
    from numpy_quant.device import DeviceArray, sync
    from numpy_quant.images import ImagePreprocess, ResizeCrop
    _lib.ensure_init()
    pre = ImagePreprocess(*IMAGENET, resize=ResizeCrop(256, 224))
    B = args.batch
    photos = _photos(B, 1)[0]
    batch = pre.pack(photos)
    host = np.empty(batch.nbytes, np.uint8)
    batch.write(host)
    out_bytes = B * 3 * 224 * 224
    moved = batch.pixel_bytes + out_bytes
    pairs = max(1, -(-(320 << 20) // moved))  # more than 256 MiB in flight
    srcs = [DeviceArray.from_host(host) for _ in range(pairs)]
    lut, _ = K.quantize(pre.table_device(), 8, np.float32(0.02), -3)
    outs = [pre.lookup_resized(s, batch, host.ctypes.data, lut) for s in srcs]
    u8 = pre.resize.reference(photos)
    want = np.stack([lut.to_host()[c][u8[..., c]] for c in range(3)], axis=1)
    for o in outs:
        if not np.array_equal(o.to_host(), want):
            raise AssertionError("nqk_image_resize_lut differs from ResizeCrop.reference + the NumPy gather")

    def kernel_round():
        for s, o in zip(srcs, outs):
            _lib.call("nqk_image_resize_lut", s.offset_view(batch.pixel_offset, (batch.pixel_bytes,)).vp, batch.pixel_bytes,
                      s.vp, ctypes.c_void_p(host.ctypes.data), batch.meta.size, lut.vp, lut.code, o.vp, B, 3, 224, 224)

    samples = []
    for i in range(args.warmup + args.rounds):
        ms = _timer_ms(lambda: [kernel_round() for _ in range(args.reps)])
        if i >= args.warmup:
            samples.append(1e3 * ms / (args.reps * pairs))
    us = statistics.median(samples)
    sync()
    return {"resize_kernel_us": round(us, 2), "resize_kernel_us_min_max": [round(min(samples), 2), round(max(samples), 2)],
            "resize_bytes_in": batch.pixel_bytes, "resize_bytes_out": out_bytes, "resize_buffer_pairs": pairs,
            "resize_TBps": round(moved / (us * 1e-6) / 1e12, 3),
            "resize_fraction_of_copy_rate": round(moved / (us * 1e-6) / COPY_RATE, 3)}


def step_resize_e2e(args) -> dict:
    from numpy_quant import _lib, onnx_proto
    from numpy_quant.images import ImagePreprocess, ResizeCrop
    from numpy_quant.model import Model
    _lib.ensure_init()
    rc = ResizeCrop(256, 224)
    pre, plain = ImagePreprocess(*IMAGENET, resize=rc), ImagePreprocess(*IMAGENET)
    B = args.batch
    lists = _photos(B, args.stream_batches)
    resized = [rc.reference(b) for b in lists]  # uint8 [B, 224, 224, 3]
    model = Model.from_onnx(onnx_proto.load(MODEL_FILE, synthetic_weights=True))
    calib = min(8, B)
    model.rebatch(calib)
    qmodel = model.quantize([plain.reference(resized[0][:calib])], bit_width=8)
    for v in model.values:  # free the float calibration activations
        if v.__class__.__name__ == "Variable":
            v.data = None
    model.rebatch(B)
    plan = qmodel.compile()

    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pillow(photos):
        rh, rw, top, left, oh, ow = rc.window(*SOURCE_HW)
        box = (left, top, left + ow, top + oh)
        return np.stack([np.asarray(Image.fromarray(p).resize((rw, rh), Image.BILINEAR).crop(box)) for p in photos])

    def run(preprocess, x):
        qmodel.image_preprocess = preprocess
        return qmodel([x])[0]

    # every row of the list path and the stream against the float32 path; Pillow against the definition
    want = [run(plain, plain.reference(r)) for r in resized]
    for b, w in zip(lists, want):
        if not np.array_equal(run(pre, b).view(np.uint32), w.view(np.uint32)):
            raise AssertionError("qmodel([list]) differs from the float32 path")
    qmodel.image_preprocess = pre
    for g, w in zip(qmodel.classify_stream(lists), want):
        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            raise AssertionError("classify_stream over lists differs from the float32 path")
    if Image is not None and not np.array_equal(pillow(lists[0]), resized[0]):
        raise AssertionError("Pillow's resize + crop differs from ResizeCrop.reference")

    def leg_list():
        for b in lists:
            run(pre, b)

    def leg_224():
        for r in resized:
            run(plain, r)

    def leg_pillow():
        for b in lists:
            run(plain, pillow(b))

    def leg_stream():
        qmodel.image_preprocess = pre
        for _ in qmodel.classify_stream(lists):
            pass

    legs = {"r_list": leg_list, "r_224": leg_224, "r_stream": leg_stream}
    if Image is not None:
        legs["r_pillow"] = leg_pillow
    samples = {k: [] for k in legs}
    for i in range(args.warmup + args.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                samples[name].append(1e3 * (time.perf_counter() - t0) / len(lists))
    res = {"fused_layers": plan.fused, "rows_verified": int(sum(w.shape[0] for w in want)) * 2,
           "pillow": "not importable here: the host recipe was not measured" if Image is None
           else f"{Image.__name__.split('.')[0]} {__import__('PIL').__version__}, byte-identical to ResizeCrop.reference"}
    for name, s in samples.items():
        res[f"{name}_ms_per_batch"] = round(statistics.median(s), 3)
        res[f"{name}_ms_min_max"] = [round(min(s), 3), round(max(s), 3)]
        res[f"{name}_images_per_s"] = round(B / (statistics.median(s) * 1e-3), 1)
    return res


STEPS = {"micro": (step_micro, 240), "e2e": (step_e2e, 420)}
RESIZE_STEPS = {"resize_micro": (step_resize_micro, 240), "resize_e2e": (step_resize_e2e, 540)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="kernel launches per buffer pair and timed window")
    ap.add_argument("--stream-batches", type=int, default=4)
    ap.add_argument("--resize", action="store_true", help="photos of 375 x 500 through ResizeCrop(256, 224) instead")
    ap.add_argument("--step", choices=sorted({**STEPS, **RESIZE_STEPS}),
                    help="run one GPU step in this process (used by the parent)")
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps({**STEPS, **RESIZE_STEPS}[args.step][0](args)), flush=True)
        return 0
    steps = RESIZE_STEPS if args.resize else STEPS
    result = {"metric": "uint8 image inputs, ViT-Base int8 (synthetic weights), host arrays in, logits out",
              "batch": args.batch, "rounds": args.rounds, "stream_batches": args.stream_batches,
              "verified": "every output row of b and c equals the float32 path's, bit for bit"}
    if args.resize:
        result["metric"] = ("uint8 photos of %d x %d, resize 256 + center crop 224 on the device, ViT-Base int8 "
                            "(synthetic weights), host arrays in, logits out" % SOURCE_HW)
        result["verified"] = "every output row of r_list and r_stream equals the float32 path's, bit for bit"
    passthrough = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("batch", "rounds", "warmup", "reps", "stream_batches")]
    for name, (_, limit) in steps.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + passthrough
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"[bench_images] step {name} ran past its {limit} s limit; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"[bench_images] step {name} failed ({p.returncode}); nothing more is started", file=sys.stderr)
            return p.returncode or 1
        result.update(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
