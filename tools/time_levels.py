#!/usr/bin/env python3
"""Timings of the level operators (levels.hip and the table path) on noise frames, gray and RGBA, Q16
and float Quantum:

  <operator>_ms        the call on a device image (hipEvents around --reps calls, the refill of the
                       frame subtracted): level1 (gamma 1: evaluated per sample), level (gamma 2.2: a
                       table on Q16, the device's pow on float), levelize (gamma 0.45), gamma, negate,
                       negate_gray, sigmoidal, sigmoidal_inverse; range (MagickHipImageRange: the scan,
                       80 bytes down, a synchronisation), auto_level (the scan, then LevelImage) and
                       linear_stretch (the intensity histogram, 512 KiB per channel down, LevelImage)
  <operator>_fraction  the operator's algorithmic bytes over its time against 8 TB/s: a pointwise
                       operator reads and writes the frame, the range scan reads it, auto_level and
                       linear_stretch read it twice and write it once
  table_build_ms       host wall time of a LevelImage call with parameters no table exists for, less
                       that of the same call repeated (Q16 only): 65536 pow calls and one upload
  cpu_*_ms             the compiled reference's wall time, on the --cpu-side frame only

    python tools/time_levels.py [--reps N] [--sides 2048,8192] [--cpu-side 2048] [--no-cpu]

One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
FRAME_PASSES = {"range": 1, "auto_level": 3, "linear_stretch": 3}       # every other operator: 2


def event_ms(call, reps):
    import torch
    call()                                               # warm-up: code object, pool, table
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def wall_ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sides", default="2048,8192")
    ap.add_argument("--cpu-side", type=int, default=2048)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch
    import imagemagick_amd as im
    from conftest import to_device
    import levels_oracle as lo
    if not torch.cuda.is_available():
        raise SystemExit("time_levels.py needs a GPU")
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not (refmod.available(False) and refmod.available(True)):
            refmod = None
    fresh = [1.3]                                        # a gamma no table exists for yet
    for side in (int(s) for s in args.sides.split(",")):
        for channels in (1, 4):
            for dtype in (np.uint16, np.float32):
                px = lo.noise(side, side, channels, dtype)
                source = to_device(px)
                work = source.clone()
                frame = im.Image(work)
                operators = {
                    "level1": lambda: im.level_image(frame, 5000.0, 60000.0, 1.0),
                    "level": lambda: im.level_image(frame, 5000.0, 60000.0, 2.2),
                    "levelize": lambda: im.levelize_image(frame, 5000.0, 60000.0, 0.45),
                    "gamma": lambda: im.gamma_image(frame, 2.2),
                    "negate": lambda: im.negate_image(frame, False),
                    "negate_gray": lambda: im.negate_image(frame, True),
                    "sigmoidal": lambda: im.sigmoidal_contrast_image(frame, True, 5.0, 32767.5),
                    "sigmoidal_inverse": lambda: im.sigmoidal_contrast_image(frame, False, 5.0, 32767.5),
                    "range": lambda: im.image_range(frame),
                    "auto_level": lambda: im.auto_level_image(frame),
                    "linear_stretch": lambda: im.linear_stretch_image(frame, 0.02 * side * side, 0.01 * side * side)}

                def refill():
                    work.copy_(source)                   # in place: every call starts from the noise frame
                copy_ms = event_ms(refill, args.reps)
                row = {"side": side, "channels": channels, "quantum": np.dtype(dtype).name, "refill_ms": round(copy_ms, 4)}
                for name, call in operators.items():
                    def one(call=call):
                        refill()
                        call()
                    ms = event_ms(one, args.reps) - copy_ms
                    row[name + "_ms"] = round(ms, 4)
                    row[name + "_fraction"] = round(FRAME_PASSES.get(name, 2) * px.nbytes / HBM_BYTES_PER_S / (ms * 1e-3), 4)
                if dtype == np.uint16:
                    def level_with(gamma):
                        im.level_image(frame, 5000.0, 60000.0, gamma)
                        torch.cuda.synchronize()
                    fresh[0] += 0.01
                    first = wall_ms(lambda: level_with(fresh[0]))
                    row["table_build_ms"] = round(first - wall_ms(lambda: level_with(fresh[0])), 4)
                if refmod is not None and side == args.cpu_side:
                    reference = {"level1": lambda i: lo.ref_level(i, 5000.0, 60000.0, 1.0),
                                 "level": lambda i: lo.ref_level(i, 5000.0, 60000.0, 2.2),
                                 "gamma": lambda i: lo.ref_gamma(i, 2.2), "negate": lambda i: lo.ref_negate(i, False),
                                 "sigmoidal": lambda i: lo.ref_sigmoidal(i, True, 5.0, 32767.5),
                                 "auto_level": lo.ref_auto_level,
                                 "linear_stretch": lambda i: lo.ref_linear_stretch(i, 0.02 * side * side, 0.01 * side * side)}
                    for name, call in reference.items():
                        image = refmod.RefImage(px)
                        row["cpu_%s_ms" % name] = round(wall_ms(lambda: call(image)), 1)
                print(json.dumps(row), flush=True)
                del frame, work, source


if __name__ == "__main__":
    main()
