#!/usr/bin/env python3
"""CLAHEImage timings on sRGB RGBA Q16 frames, default 0 x 0 tiles, 128 bins, clip limit 2.0, on a
noise frame and on a constant one (every lane counts the same bin):

  call_ms         the whole MagickHipCLAHEImage call on a device image (hipEvents around --reps calls)
  to_lab_ms       MagickHipTransformImageColorspace(Lab) in MH_PRECISION_EXACT on the same frame
  from_lab_ms     ... and back
  histogram_ms    the three kernels alone (the library's own hipEvent records around them)
  map_ms
  interpolate_ms
  *_fraction      each stage's algorithmic bytes over its time against 8 TB/s: the conversions read
                  and write the frame; the histogram reads channel 0 (2 of every 8 bytes), the
                  interpolation reads and writes it; the map kernel touches tiles x bins x 6 bytes
  cpu_ms          the compiled reference's wall time, on the --cpu-side frame only

    python tools/time_clahe.py [--reps N] [--sides 2048,8192] [--cpu-side 2048] [--no-cpu]

One JSON line per case, then a table."""
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

BINS, CLIP = 128, 2.0
HBM_BYTES_PER_S = 8.0e12
STAGES = ["to_lab", "histogram", "map", "interpolate", "from_lab"]


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


def kernel_ms(lib, _lib, call, reps):
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
    missing = [name for name in ("clahe_histogram", "clahe_map", "clahe_interpolate") if name not in out]
    if missing:
        raise RuntimeError("no profile record for %s" % missing)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sides", default="2048,8192")
    ap.add_argument("--cpu-side", type=int, default=2048)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch
    import imagemagick_amd as im
    from imagemagick_amd import _lib
    from conftest import to_device
    from clahe_oracle import noise, constant, ref_clahe
    if not torch.cuda.is_available():
        raise SystemExit("time_clahe.py needs a GPU")
    lib = _lib.load()
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not refmod.available(False):
            refmod = None
    rows = []
    for side in (int(s) for s in args.sides.split(",")):
        for kind, make in (("noise", noise), ("constant", constant)):
            px = make(side, side, 4, np.uint16)
            source = to_device(px)
            work = source.clone()
            frame = im.Image(work)
            exact = im.Image(work, precision=im.PRECISION_EXACT)

            def call():
                work.copy_(source)                       # in place: every call starts from the sRGB frame
                d = frame.descriptor()
                _lib.check(lib.MagickHipCLAHEImage(ctypes.byref(d), 0, 0, BINS, CLIP))

            def copy():
                work.copy_(source)

            def to_lab():
                d = exact.descriptor()
                d.colorspace = _lib.COLORSPACES["srgb"]
                _lib.check(lib.MagickHipTransformImageColorspace(ctypes.byref(d), _lib.COLORSPACES["lab"]))

            def from_lab():
                d = exact.descriptor()
                d.colorspace = _lib.COLORSPACES["lab"]
                _lib.check(lib.MagickHipTransformImageColorspace(ctypes.byref(d), _lib.COLORSPACES["srgb"]))
            copy_ms = event_ms(copy, args.reps)
            row = {"side": side, "frame": kind, "call_ms": round(event_ms(call, args.reps) - copy_ms, 4),
                   "to_lab_ms": round(event_ms(to_lab, args.reps), 4), "from_lab_ms": round(event_ms(from_lab, args.reps), 4)}
            records = kernel_ms(lib, _lib, call, args.reps)
            for stage in ("histogram", "map", "interpolate"):
                row[stage + "_ms"] = round(records["clahe_" + stage], 4)
            tw, th = side >> 3, side >> 3
            tiles = ((side + tw - 1) // tw) * ((side + th - 1) // th)
            pixels = side * side
            stage_bytes = {"to_lab": 2 * px.nbytes, "from_lab": 2 * px.nbytes, "histogram": 2 * pixels,
                           "interpolate": 4 * pixels, "map": tiles * BINS * 6}
            for stage in STAGES:
                row[stage + "_fraction"] = round(stage_bytes[stage] / HBM_BYTES_PER_S / (row[stage + "_ms"] * 1e-3), 4)
            if refmod is not None and side == args.cpu_side:
                image = refmod.RefImage(px)
                t = time.perf_counter()
                ref_clahe(image, 0, 0, BINS, CLIP)
                row["cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del frame, exact, work, source
    print("\n%6s %-9s %9s " % ("side", "frame", "call_ms") + " ".join("%16s" % s for s in STAGES) + " %9s" % "cpu_ms")
    for r in rows:
        print("%6d %-9s %9.3f " % (r["side"], r["frame"], r["call_ms"]) +
              " ".join("%9.3f (%4.1f%%)" % (r[s + "_ms"], 100.0 * r[s + "_fraction"]) for s in STAGES) +
              " %9s" % r.get("cpu_ms", "-"))


if __name__ == "__main__":
    main()
