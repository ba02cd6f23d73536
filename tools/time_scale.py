#!/usr/bin/env python3
"""Timings of ScaleImage and ThumbnailImage (scale.hip) on RGBA noise frames, Q16 and float Quantum:

  scale      8192^2 -> 2048^2, 8192^2 -> 819^2 and 2048^2 -> 8192^2:
             scale_ms        MagickHipScaleImage on a device image (hipEvents around --reps calls)
             box_resize_ms   this library's ResizeImage(Box) at the same geometry, in the library's
                             default mode (FAST)
             fraction        the compulsory bytes (source read once, destination written once) over
                             scale_ms against 8 TB/s
             cpu_scale_ms    the compiled reference's ScaleImage, wall time (single-threaded there)
  thumbnail  8192^2 -> 256^2:
             thumbnail_ms    MagickHipThumbnailImage
             sample_ms, box_ms, final_ms   its three stages called one by one
             cpu_thumbnail_ms              the compiled reference's ThumbnailImage

    python tools/time_scale.py [--reps N] [--no-cpu] [--small]

--small divides every side by 8 (a quick check of the tool itself).  One JSON line per case."""
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
SCALES = [(8192, 2048), (8192, 819), (2048, 8192)]
THUMBNAIL = (8192, 256)


def event_ms(call, reps):
    import torch
    call()                                               # warm-up: code object, pool, tables
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def to_device(array):
    import torch
    if array.dtype == np.uint16:
        return torch.from_numpy(array.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(array).cuda()


def wall_ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()

    import torch
    import imagemagick_amd as im
    import scale_oracle as so
    if not torch.cuda.is_available():
        raise SystemExit("time_scale.py needs a GPU")
    im.load()
    refmod = None
    if not args.no_cpu:
        from oracle import ref as refmod
        if not (refmod.available(False) and refmod.available(True)):
            refmod = None
    shrink = 8 if args.small else 1
    sources = {}

    def source(side, dtype):
        key = (side, np.dtype(dtype).name)
        if key not in sources:
            sources.clear()                              # one big frame at a time
            sources[key] = so.frame("rgba", side, side, dtype, seed=11)
        return sources[key]

    for dtype in (np.uint16, np.float32):
        for side, to in SCALES:
            side, to = side // shrink, max(to // shrink, 1)
            px = source(side, dtype)
            image = im.Image(to_device(px))
            row = {"case": "scale", "side": side, "to": to, "quantum": np.dtype(dtype).name}
            row["scale_ms"] = round(event_ms(lambda: im.scale_image(image, to, to), args.reps), 4)
            row["box_resize_ms"] = round(event_ms(lambda: im.resize_image(image, to, to, "box"), args.reps), 4)
            compulsory = px.nbytes + to * to * 4 * px.itemsize
            row["fraction"] = round(compulsory / HBM_BYTES_PER_S / (row["scale_ms"] * 1e-3), 4)
            if refmod is not None:
                reference = refmod.RefImage(px)
                row["cpu_scale_ms"] = round(wall_ms(lambda: so.ref_scale(refmod, reference, to, to)), 1)
            print(json.dumps(row), flush=True)
            del image
        side, to = THUMBNAIL[0] // shrink, max(THUMBNAIL[1] // shrink, 1)
        px = source(side, dtype)
        image = im.Image(to_device(px))
        row = {"case": "thumbnail", "side": side, "to": to, "quantum": np.dtype(dtype).name}
        row["thumbnail_ms"] = round(event_ms(lambda: im.thumbnail_image(image, to, to), args.reps), 4)
        sampled = im.sample_image(image, 4 * to, 4 * to)
        boxed = im.resize_image(sampled, 2 * to, 2 * to, "box")
        row["sample_ms"] = round(event_ms(lambda: im.sample_image(image, 4 * to, 4 * to), args.reps), 4)
        row["box_ms"] = round(event_ms(lambda: im.resize_image(sampled, 2 * to, 2 * to, "box"), args.reps), 4)
        row["final_ms"] = round(event_ms(lambda: im.resize_image(boxed, to, to, "lanczossharp"), args.reps), 4)
        if refmod is not None:
            reference = refmod.RefImage(px)
            row["cpu_thumbnail_ms"] = round(wall_ms(lambda: so.ref_thumbnail(refmod, reference, to, to)), 1)
        print(json.dumps(row), flush=True)
        del image, sampled, boxed


if __name__ == "__main__":
    main()
