#!/usr/bin/env python3
"""Child process of tests/test_gpu_threshold_shim.py: a FRESH process - no MAGICK_HIP_PRECISION /
MAGICKHIP_* in the environment, no MhSetPrecision call, so the library runs in its default FAST mode -
drives MagickCore's own AdaptiveThresholdImage, BilevelImage and AutoThresholdImage through the
HIP-backed build the way an unchanged caller does and compares every sample, the colourspace and the
auto-threshold:threshold property with the plain compiled reference.  Prints one JSON object."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import ref as refmod
from statistic_oracle import set_virtual_pixels, TILE_VIRTUAL_PIXELS
from threshold_oracle import (noise, ref_image, ref_bilevel, ref_auto_threshold, ref_adaptive_threshold, METHODS)

for name in list(os.environ):
    if name.startswith("MAGICKHIP_") or name == "MAGICK_HIP_PRECISION":
        del os.environ[name]
os.environ["MAGICK_HIP_LIBRARY"] = os.path.join(ROOT, "imagemagick_amd", "lib", "libmagickhip.so")


class Record(ctypes.Structure):
    _fields_ = [("kernel_name", ctypes.c_char_p), ("count", ctypes.c_ulong), ("min_ms", ctypes.c_double),
                ("max_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


def calls(hdri):
    lib = refmod._load(hdri, True)
    lib.GetMagickHipAcceleratedCalls.restype = ctypes.c_size_t
    return lib.GetMagickHipAcceleratedCalls()


def differing(got, want):
    return int((got.view(np.uint8) != want.view(np.uint8)).sum())


def run(px, operator, colorspace="sRGB", prepare=None):
    """operator(image) -> (result image, property or None) on the CPU build and on the HIP-backed one."""
    hdri = px.dtype == np.float32
    cpu_image = ref_image(refmod, px, colorspace)
    gpu_image = ref_image(refmod, px, colorspace, shim=True)
    if prepare is not None:
        prepare(cpu_image)
        prepare(gpu_image)
    cpu, cpu_property = operator(cpu_image)
    before = calls(hdri)
    gpu, gpu_property = operator(gpu_image)
    return {"accelerated": calls(hdri) - before, "differing": differing(gpu.numpy(), cpu.numpy()),
            "changed": differing(gpu.numpy(), px), "colorspace": gpu.info()["colorspace"],
            "cpu_colorspace": cpu.info()["colorspace"], "property": gpu_property, "cpu_property": cpu_property}


def adaptive(width, height, bias):
    return lambda image: (ref_adaptive_threshold(refmod, image, width, height, bias), None)


def bilevel(threshold):
    return lambda image: (ref_bilevel(image, threshold), None)


def auto(method):
    return lambda image: ref_auto_threshold(image, method)


# the library instance the shim loads (one per path): its profile records show which kernels ran
_ = calls(False)
hip = ctypes.CDLL(os.environ["MAGICK_HIP_LIBRARY"])
hip.MhGetPrecision.restype = ctypes.c_int
hip.MhGetProfileRecords.restype = ctypes.c_size_t
hip.MhGetProfileRecords.argtypes = [ctypes.POINTER(Record), ctypes.c_size_t]
hip.MhResetProfileRecords()
hip.MhSetProfileEnabled(1)

Q16, HDRI = np.uint16, np.float32
report = {"adaptive": [], "bilevel": [], "auto": []}
report["adaptive"].append(run(noise(61, 97, 4, Q16), adaptive(7, 5, -655.35)))
report["adaptive"].append(run(noise(61, 97, 1, Q16), adaptive(25, 25, 1966.05), "Gray"))
report["adaptive"].append(run(noise(33, 97, 3, HDRI), adaptive(9, 9, 0.25)))
report["bilevel"].append(run(noise(61, 97, 4, Q16), bilevel(30000.25)))
report["bilevel"].append(run(noise(61, 97, 3, HDRI), bilevel(28000.5), "RGB"))       # retagged sRGB
report["bilevel"].append(run(noise(61, 97, 2, Q16), bilevel(float(noise(61, 97, 2, Q16)[5, 5, 0])), "Gray"))
for i, method in enumerate(METHODS):
    report["auto"].append(run(noise(61, 97, (4, 1, 3)[i], (Q16, HDRI, Q16)[i]), auto(method), ("sRGB", "Gray", "RGB")[i]))
# a window over the library's limit: declined inside the library, MagickCore's own code answers
report["wide"] = run(noise(40, 50, 3, Q16), adaptive(300, 3, 0.0))
# virtual pixels the library cannot see: the hook's gate declines
report["tile"] = run(noise(40, 50, 3, Q16), adaptive(7, 7, 0.0),
                     prepare=lambda image: set_virtual_pixels(refmod, image, TILE_VIRTUAL_PIXELS))

hip.MhSetProfileEnabled(0)
records = (Record * 64)()
n = hip.MhGetProfileRecords(records, 64)
report["kernels"] = sorted({records[i].kernel_name.decode() for i in range(min(n, 64))})
# what mode was that?  (asked LAST; nobody set it)
report["precision"] = int(hip.MhGetPrecision())
print(json.dumps(report))
