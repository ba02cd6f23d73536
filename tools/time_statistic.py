#!/usr/bin/env python3
"""StatisticImage timings: the device kernel of every type for windows 3, 5, 7, 15 and 31 on a
4096 x 4096 RGBA and gray Q16 frame, and the compiled reference on a smaller frame, scaled per pixel.

    python tools/time_statistic.py [--reps N] [--types Median,Mean] [--windows 3,5] [--no-cpu]

Kernel time: the library's own hipEvent records (MhSetProfileEnabled / MhGetProfileRecords) around
the statistic kernel, averaged over --reps calls after one warm-up call.  GB/s: the frame read once
and written once over that time.  The mode's distinct-key walk on random data costs about n^2 LDS
reads an output at n = W*H > 32; its 15 and 31 cases run on a 1024 x 1024 frame and are scaled up
to 4096 x 4096 (marked "scaled").  One JSON line per case, then a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TYPES = ["Gradient", "Maximum", "Mean", "Median", "Minimum", "Mode", "NonPeak", "RootMeanSquare",
         "StandardDeviation", "Contrast"]


def device_ms(im, lib, _lib, image, statistic, window, reps):
    import torch
    im.statistic_image(image, statistic, window, window)          # warm-up: code object, pool
    torch.cuda.synchronize()
    lib.MhResetProfileRecords()
    lib.MhSetProfileEnabled(1)
    for _ in range(reps):
        im.statistic_image(image, statistic, window, window)
    torch.cuda.synchronize()
    lib.MhSetProfileEnabled(0)
    records = (_lib.MhKernelProfileRecord * 48)()
    n = lib.MhGetProfileRecords(records, 48)
    out = {}
    for i in range(min(n, 48)):
        r = records[i]
        name = r.kernel_name.decode()
        if name.startswith("statistic_"):
            out[name] = r.total_ms / max(int(r.count), 1)
    lib.MhResetProfileRecords()
    if len(out) != 1:
        raise RuntimeError("expected one statistic kernel, got %s" % out)
    return out.popitem()


def cpu_ms(refmod, statistic, window, channels, side):
    from statistic_oracle import ref_statistic
    from conftest import make_pixels
    px = make_pixels(side, side, channels, np.uint16, seed=3)
    image = refmod.RefImage(px)
    t = time.perf_counter()
    ref_statistic(refmod, image, statistic, window, window)
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--types", default=",".join(TYPES))
    ap.add_argument("--windows", default="3,5,7,15,31")
    ap.add_argument("--channels", default="4,1")
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch
    import imagemagick_amd as im
    from imagemagick_amd import _lib
    from conftest import make_pixels, to_device
    if not torch.cuda.is_available():
        raise SystemExit("time_statistic.py needs a GPU")
    lib = _lib.load()
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not refmod.available(False):
            refmod = None
    rows = []
    for channels in [int(c) for c in args.channels.split(",")]:
        frames = {}
        for statistic in args.types.split(","):
            for window in [int(w) for w in args.windows.split(",")]:
                side = args.side
                if statistic == "Mode" and window * window > 32 and window >= 15:
                    side = min(side, 1024)
                if side not in frames:
                    frames[side] = im.Image(to_device(make_pixels(side, side, channels, np.uint16, seed=1)))
                route, ms = device_ms(im, lib, _lib, frames[side], statistic, window, args.reps)
                scale = (args.side / side) ** 2
                ms *= scale
                nbytes = 2.0 * args.side * args.side * channels * 2
                row = {"type": statistic, "window": window, "channels": channels, "side": args.side,
                       "route": route, "kernel_ms": round(ms, 4), "gbps": round(nbytes / (ms * 1e6), 1),
                       "scaled_from": side if side != args.side else None}
                if refmod is not None:
                    cpu_side = 256 if window <= 7 else 128
                    c = cpu_ms(refmod, statistic, window, channels, cpu_side)
                    row["cpu_ms_scaled"] = round(c * (args.side / cpu_side) ** 2, 1)
                    row["speedup"] = round(row["cpu_ms_scaled"] / ms, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("\n%-18s %3s %2s %-22s %10s %8s %12s %9s" % ("type", "win", "ch", "route", "kernel_ms", "GB/s",
                                                        "cpu_ms", "speedup"))
    for r in rows:
        print("%-18s %3d %2d %-22s %10.3f %8.1f %12s %9s" % (
            r["type"], r["window"], r["channels"], r["route"], r["kernel_ms"], r["gbps"],
            r.get("cpu_ms_scaled", "-"), r.get("speedup", "-")) + (" (scaled)" if r["scaled_from"] else ""))


if __name__ == "__main__":
    main()
