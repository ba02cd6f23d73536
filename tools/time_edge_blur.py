#!/usr/bin/env python3
"""BilateralBlurImage and SelectiveBlurImage timings: the device kernels on a 4096 x 4096 RGBA frame,
Q16 and float Quantum (bilateral 5x5, 9x9, 15x15 at sigmas 20 / 3; selective sigma 1.5, 2, 4 at a
threshold of 10 %), and the compiled reference on a 1024 x 1024 crop, scaled by pixel count.

    python tools/time_edge_blur.py [--reps N] [--side 4096] [--cpu-side 1024] [--no-cpu]

Kernel time: the library's own hipEvent records (MhSetProfileEnabled / MhGetProfileRecords) around
the kernel, averaged over --reps calls after one warm-up call.  The reference's time is wall time on
this box's CPU threads (printed).  One JSON line per case, then a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("bilateral", (5, 5, 20.0, 3.0)), ("bilateral", (9, 9, 20.0, 3.0)), ("bilateral", (15, 15, 20.0, 3.0)),
         ("selective", (0.0, 1.5, 6553.5)), ("selective", (0.0, 2.0, 6553.5)), ("selective", (0.0, 4.0, 6553.5))]


def device_ms(im, lib, _lib, image, operator, args, reps):
    import torch
    call = im.bilateral_blur_image if operator == "bilateral" else im.selective_blur_image
    call(image, *args)                                   # warm-up: code object, pool
    torch.cuda.synchronize()
    lib.MhResetProfileRecords()
    lib.MhSetProfileEnabled(1)
    for _ in range(reps):
        call(image, *args)
    torch.cuda.synchronize()
    lib.MhSetProfileEnabled(0)
    records = (_lib.MhKernelProfileRecord * 48)()
    n = lib.MhGetProfileRecords(records, 48)
    out = {}
    for i in range(min(n, 48)):
        r = records[i]
        name = r.kernel_name.decode()
        if name.startswith(operator + "_"):
            out[name] = r.total_ms / max(int(r.count), 1)
    lib.MhResetProfileRecords()
    if len(out) != 1:
        raise RuntimeError("expected one %s kernel, got %s" % (operator, out))
    return out.popitem()[1]


def cpu_ms(refmod, px, operator, args):
    from edge_blur_oracle import ref_bilateral, ref_selective
    image = refmod.RefImage(px)
    t = time.perf_counter()
    (ref_bilateral if operator == "bilateral" else ref_selective)(refmod, image, *args)
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--cpu-side", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch
    import imagemagick_amd as im
    from imagemagick_amd import _lib
    from conftest import make_pixels, to_device
    if not torch.cuda.is_available():
        raise SystemExit("time_edge_blur.py needs a GPU")
    lib = _lib.load()
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not (refmod.available(False) and refmod.available(True)):
            refmod = None
    rows = []
    for dtype in (np.uint16, np.float32):
        px = np.maximum(make_pixels(args.side, args.side, 4, dtype, seed=1, kind="smooth"), dtype(300))
        frame = im.Image(to_device(px))
        crop = np.ascontiguousarray(px[:args.cpu_side, :args.cpu_side])
        for operator, parameters in CASES:
            ms = device_ms(im, lib, _lib, frame, operator, parameters, args.reps)
            row = {"operator": operator, "args": list(parameters), "quantum": np.dtype(dtype).name, "side": args.side,
                   "kernel_ms": round(ms, 4), "mpix_per_s": round(args.side * args.side / (ms * 1e3), 1)}
            if refmod is not None:
                c = cpu_ms(refmod, crop, operator, parameters)
                row["cpu_threads"] = refmod.thread_limit(dtype == np.float32)
                row["cpu_ms_scaled"] = round(c * (args.side / args.cpu_side) ** 2, 1)
                row["speedup"] = round(row["cpu_ms_scaled"] / ms, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n%-10s %-24s %-8s %10s %10s %12s %9s" % ("operator", "args", "quantum", "kernel_ms", "Mpix/s", "cpu_ms",
                                                    "speedup"))
    for r in rows:
        print("%-10s %-24s %-8s %10.3f %10.1f %12s %9s" % (
            r["operator"], "x".join("%g" % a for a in r["args"]), r["quantum"], r["kernel_ms"], r["mpix_per_s"],
            r.get("cpu_ms_scaled", "-"), r.get("speedup", "-")))


if __name__ == "__main__":
    main()
