#!/usr/bin/env python3
"""Child process of tests/test_gpu_kuwahara_shim.py: a FRESH process - no MAGICK_HIP_PRECISION /
MAGICKHIP_* in the environment, no MhSetPrecision call, so the library runs in its default FAST mode -
drives MagickCore's own KuwaharaImage through the HIP-backed build the way an unchanged caller does
and compares every sample with the plain compiled reference.  Prints one JSON object."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import ref as refmod
from kuwahara_oracle import noise, sprite_alpha, ref_kuwahara, set_interpolate

for name in list(os.environ):
    if name.startswith("MAGICKHIP_") or name == "MAGICK_HIP_PRECISION":
        del os.environ[name]
os.environ["MAGICK_HIP_LIBRARY"] = os.path.join(ROOT, "imagemagick_amd", "lib", "libmagickhip.so")


def calls(hdri):
    lib = refmod._load(hdri, True)
    lib.GetMagickHipAcceleratedCalls.restype = ctypes.c_size_t
    return lib.GetMagickHipAcceleratedCalls()


def differing(got, want):
    return int((got.view(np.uint8) != want.view(np.uint8)).sum())


report = {"cases": []}
for dtype in (np.uint16, np.float32):
    hdri = dtype == np.float32
    for channels, radius, sigma in [(4, 2, 1.5), (4, 3, 3.0), (3, 1, 0.5), (1, 4, 1.5), (2, 2, 1.5)]:
        px = noise(70, 90, channels, dtype)
        if channels in (2, 4):
            px = sprite_alpha(px)
        cpu = ref_kuwahara(refmod, refmod.RefImage(px), radius, sigma).numpy()
        before = calls(hdri)
        gpu = ref_kuwahara(refmod, refmod.RefImage(px, shim=True), radius, sigma).numpy()
        report["cases"].append({"quantum": np.dtype(dtype).name, "channels": channels, "radius": radius,
                                "sigma": sigma, "accelerated": calls(hdri) - before,
                                "differing": differing(gpu, cpu), "changed": differing(gpu, px)})
    # image->interpolate = Nearest: the hook declines, MagickCore's own code answers
    px = noise(40, 50, 4, dtype)
    before = calls(hdri)
    gpu = ref_kuwahara(refmod, set_interpolate(refmod.RefImage(px, shim=True), "Nearest"), 2, 1.5).numpy()
    cpu = ref_kuwahara(refmod, set_interpolate(refmod.RefImage(px), "Nearest"), 2, 1.5).numpy()
    bilinear = ref_kuwahara(refmod, refmod.RefImage(px), 2, 1.5).numpy()
    report["nearest_" + np.dtype(dtype).name] = {"accelerated": calls(hdri) - before, "differing": differing(gpu, cpu),
                                                 "differs_from_bilinear": differing(cpu, bilinear)}

# a radius beyond the library's window limit (float Quantum RGBA: w <= 27): declined inside the library
px = noise(40, 50, 4, np.float32)
before = calls(True)
gpu = ref_kuwahara(refmod, refmod.RefImage(px, shim=True), 30, 1.5).numpy()
report["over_the_limit"] = {"accelerated": calls(True) - before,
                            "differing": differing(gpu, ref_kuwahara(refmod, refmod.RefImage(px), 30, 1.5).numpy())}

# what mode was that?  (asked LAST, through the library instance the shim loaded; nobody set it)
hip = ctypes.CDLL(os.environ["MAGICK_HIP_LIBRARY"])
hip.MhGetPrecision.restype = ctypes.c_int
report["precision"] = int(hip.MhGetPrecision())
print(json.dumps(report))
