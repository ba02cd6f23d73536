#!/usr/bin/env python3
"""Timings of the threshold operators (threshold.hip) on noise frames, gray and RGBA, Q16 and float
Quantum:

  bilevel_ms       MagickHipBilevelImage on a device image (hipEvents around --reps calls)
  auto_ms          MagickHipAutoThresholdImage (OTSU): histogram kernel, 2 KiB down, host selection, bilevel
  histogram_ms     the histogram kernel alone (the library's own hipEvent record)
  lat<W>_ms        MagickHipAdaptiveThresholdImage with a W x W window, bias -3 % (the kernel's record;
                   lat<W>_call_ms the whole call)
  *_fraction       the stage's algorithmic bytes over its time against 8 TB/s: bilevel reads and writes
                   the frame, the histogram reads it, AdaptiveThreshold reads it twice (entering and
                   leaving rows) and writes it once
  cpu_*_ms         the compiled reference's wall time, on the --cpu-side frame only

    python tools/time_threshold.py [--reps N] [--sides 2048,8192] [--cpu-side 2048] [--no-cpu] [--windows 5,25,101]
                                   [--float-lat-side 2048]

One JSON line per case."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
BIAS = -0.03 * 65535.0


def event_ms(call, reps):
    import torch
    call()                                               # warm-up: code object, pool
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def kernel_ms(lib, _lib, call, reps, name):
    import torch
    lib.MhResetProfileRecords()
    lib.MhSetProfileEnabled(1)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    lib.MhSetProfileEnabled(0)
    records = (_lib.MhKernelProfileRecord * 48)()
    n = lib.MhGetProfileRecords(records, 48)
    out = {records[i].kernel_name.decode(): records[i].total_ms / max(int(records[i].count), 1) for i in range(min(n, 48))}
    lib.MhResetProfileRecords()
    if name not in out:
        raise RuntimeError("no profile record for %s: %s" % (name, sorted(out)))
    return out[name]


def wall_ms(call):
    t = time.perf_counter()
    call()
    return round((time.perf_counter() - t) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sides", default="2048,8192")
    ap.add_argument("--cpu-side", type=int, default=2048)
    ap.add_argument("--windows", default="5,25,101")
    ap.add_argument("--float-lat-side", type=int, default=2048,
                    help="the largest frame side the float-Quantum AdaptiveThreshold is timed on: one lane walks a "
                         "whole row, W x W loads per output, so 8192^2 with 101 x 101 takes minutes")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch
    import imagemagick_amd as im
    from imagemagick_amd import _lib
    from conftest import to_device
    from threshold_oracle import noise, ref_bilevel, ref_auto_threshold, ref_adaptive_threshold
    if not torch.cuda.is_available():
        raise SystemExit("time_threshold.py needs a GPU")
    lib = _lib.load()
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not (refmod.available(False) and refmod.available(True)):
            refmod = None
    windows = [int(w) for w in args.windows.split(",")]
    for side in (int(s) for s in args.sides.split(",")):
        for channels in (1, 4):
            for dtype in (np.uint16, np.float32):
                px = noise(side, side, channels, dtype)
                source = to_device(px)
                work = source.clone()
                frame, result = im.Image(work), im.Image(torch.empty_like(source))

                def copy():
                    work.copy_(source)

                def bilevel():
                    work.copy_(source)                   # in place: every call starts from the noise frame
                    _lib.check(lib.MagickHipBilevelImage(ctypes.byref(frame.descriptor()), 30000.25))

                def auto():
                    work.copy_(source)
                    _lib.check(lib.MagickHipAutoThresholdImage(ctypes.byref(frame.descriptor()), 2, None))
                copy_ms = event_ms(copy, args.reps)
                row = {"side": side, "channels": channels, "quantum": np.dtype(dtype).name,
                       "bilevel_ms": round(event_ms(bilevel, args.reps) - copy_ms, 4),
                       "auto_ms": round(event_ms(auto, args.reps) - copy_ms, 4),
                       "histogram_ms": round(kernel_ms(lib, _lib, auto, args.reps, "threshold_histogram"), 4)}
                row["bilevel_fraction"] = round(2 * px.nbytes / HBM_BYTES_PER_S / (row["bilevel_ms"] * 1e-3), 4)
                row["histogram_fraction"] = round(px.nbytes / HBM_BYTES_PER_S / (row["histogram_ms"] * 1e-3), 4)
                record = "adaptive_threshold_q16" if dtype == np.uint16 else "adaptive_threshold_float"
                for w in (windows if dtype == np.uint16 or side <= args.float_lat_side else []):
                    def lat():
                        _lib.check(lib.MagickHipAdaptiveThresholdImage(ctypes.byref(frame.descriptor()),
                                                                       ctypes.byref(result.descriptor()), w, w, BIAS))
                    copy()
                    reps = args.reps if dtype == np.uint16 else 1
                    row["lat%d_call_ms" % w] = round(event_ms(lat, reps), 4)
                    row["lat%d_ms" % w] = round(kernel_ms(lib, _lib, lat, reps, record), 4)
                    row["lat%d_fraction" % w] = round(3 * px.nbytes / HBM_BYTES_PER_S / (row["lat%d_ms" % w] * 1e-3), 4)
                if refmod is not None and side == args.cpu_side:
                    first, second = refmod.RefImage(px), refmod.RefImage(px)
                    row["cpu_bilevel_ms"] = wall_ms(lambda: ref_bilevel(first, 30000.25))
                    row["cpu_auto_ms"] = wall_ms(lambda: ref_auto_threshold(second, "OTSU"))
                    for w in windows:
                        image = refmod.RefImage(px)
                        row["cpu_lat%d_ms" % w] = wall_ms(lambda: ref_adaptive_threshold(refmod, image, w, w, BIAS))
                print(json.dumps(row), flush=True)
                del frame, result, work, source


if __name__ == "__main__":
    main()
