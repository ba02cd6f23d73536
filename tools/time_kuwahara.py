#!/usr/bin/env python3
"""KuwaharaImage timings on RGBA frames, Q16 and float Quantum, radius 2 and 5 at sigma 1.5:

  call_ms      the whole MagickHipKuwaharaImage call on a device image (hipEvents around --reps calls)
  kernel_ms    the selection kernel alone (the library's own hipEvent records around it)
  blur_ms      MagickHipBlurImage in MH_PRECISION_EXACT on the same frame: the part no Kuwahara can avoid
  hbm_fraction the selection kernel against the HBM roofline on its compulsory traffic, one frame
               read and one written, at 6.3 TB/s (the measured float4 copy rate of an MI355X)
  cpu_ms       the compiled reference's wall time, on the --cpu-side frame only

    python tools/time_kuwahara.py [--reps N] [--sides 2048,8192] [--cpu-side 2048] [--no-cpu]

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

RADII = [2, 5]
SIGMA = 1.5
HBM_BYTES_PER_S = 6.3e12


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
    out = [records[i].total_ms / max(int(records[i].count), 1) for i in range(min(n, 48))
           if records[i].kernel_name.decode() == "kuwahara"]
    lib.MhResetProfileRecords()
    if len(out) != 1:
        raise RuntimeError("expected one kuwahara record, got %d" % len(out))
    return out[0]


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
    from kuwahara_oracle import noise, ref_kuwahara
    if not torch.cuda.is_available():
        raise SystemExit("time_kuwahara.py needs a GPU")
    lib = _lib.load()
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not (refmod.available(False) and refmod.available(True)):
            refmod = None
    rows = []
    for side in (int(s) for s in args.sides.split(",")):
        for dtype in (np.uint16, np.float32):
            px = noise(side, side, 4, dtype)
            frame = im.Image(to_device(px))
            exact = im.Image(frame.pixels, precision=im.PRECISION_EXACT)
            result = frame.like()
            for radius in RADII:
                def call():
                    src, dst = frame.descriptor(), result.descriptor()
                    _lib.check(lib.MagickHipKuwaharaImage(ctypes.byref(src), ctypes.byref(dst), float(radius), SIGMA))

                def blur():
                    src, dst = exact.descriptor(), result.descriptor()
                    _lib.check(lib.MagickHipBlurImage(ctypes.byref(src), ctypes.byref(dst), float(radius), SIGMA))
                row = {"side": side, "quantum": np.dtype(dtype).name, "radius": radius, "sigma": SIGMA,
                       "call_ms": round(event_ms(call, args.reps), 4), "blur_ms": round(event_ms(blur, args.reps), 4)}
                row["kernel_ms"] = round(kernel_ms(lib, _lib, call, args.reps), 4)
                row["hbm_fraction"] = round(2.0 * px.nbytes / HBM_BYTES_PER_S / (row["kernel_ms"] * 1e-3), 3)
                if refmod is not None and side == args.cpu_side:
                    image = refmod.RefImage(px)
                    t = time.perf_counter()
                    ref_kuwahara(refmod, image, radius, SIGMA)
                    row["cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                    row["cpu_threads"] = refmod.thread_limit(dtype == np.float32)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del frame, exact, result
    print("\n%6s %-8s %6s %10s %10s %10s %8s %10s" % ("side", "quantum", "radius", "call_ms", "kernel_ms", "blur_ms",
                                                      "hbm", "cpu_ms"))
    for r in rows:
        print("%6d %-8s %6g %10.3f %10.3f %10.3f %8.3f %10s" % (r["side"], r["quantum"], r["radius"], r["call_ms"],
                                                               r["kernel_ms"], r["blur_ms"], r["hbm_fraction"],
                                                               r.get("cpu_ms", "-")))


if __name__ == "__main__":
    main()
