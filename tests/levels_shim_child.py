#!/usr/bin/env python3
"""Child process of tests/test_gpu_levels_shim.py: a FRESH process - no MAGICK_HIP_PRECISION /
MAGICKHIP_* in the environment, no MhSetPrecision call, so the library runs in its default FAST mode -
drives MagickCore's own LevelImage, LevelizeImage, GammaImage, NegateImage, SigmoidalContrastImage,
LinearStretchImage, MinMaxStretchImage and AutoLevelImage through the HIP-backed build the way an unchanged
caller does and compares every sample, image->gamma and the histogram:linear-stretch property with the
plain compiled reference.  Prints one JSON object."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import ref as refmod
from levels_oracle import (noise, ref_image, get_property, ref_level, ref_levelize, ref_gamma, ref_negate, ref_sigmoidal,
                           ref_min_max_stretch, ref_auto_level, ref_linear_stretch, gray_pixels, _bind)

for name in list(os.environ):
    if name.startswith("MAGICKHIP_") or name == "MAGICK_HIP_PRECISION":
        del os.environ[name]
os.environ["MAGICK_HIP_LIBRARY"] = os.path.join(ROOT, "imagemagick_amd", "lib", "libmagickhip.so")
WRITE_PIXEL_MASK = 2                     # PixelMask, MagickCore/pixel.h:142


class Record(ctypes.Structure):
    _fields_ = [("kernel_name", ctypes.c_char_p), ("count", ctypes.c_ulong), ("min_ms", ctypes.c_double),
                ("max_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


def calls(hdri):
    lib = refmod._load(hdri, True)
    lib.GetMagickHipAcceleratedCalls.restype = ctypes.c_size_t
    return lib.GetMagickHipAcceleratedCalls()


def differing(got, want):
    return int((got.view(np.uint8) != want.view(np.uint8)).sum())


def image_gamma(image):
    """image->gamma as the %[gamma] escape formats it."""
    L = _bind(image.L)
    L.InterpretImageProperties.restype = ctypes.c_void_p
    L.InterpretImageProperties.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    L.DestroyString.restype = ctypes.c_void_p
    L.DestroyString.argtypes = [ctypes.c_void_p]
    exception, info = L.AcquireExceptionInfo(), L.AcquireImageInfo()
    text = L.InterpretImageProperties(info, image.handle, b"%[gamma]", exception)
    value = ctypes.string_at(text).decode()
    L.DestroyString(text)
    L.DestroyImageInfo(info)
    L.DestroyExceptionInfo(exception)
    return value


def write_mask(shim):
    """Half of the frame is write-protected: a channel the library cannot see, the hook's gate declines."""
    def prepare(image):
        L = _bind(image.L)
        info = image.info()
        protect = np.zeros((info["rows"], info["columns"], 1), dtype=np.float32 if image.hdri else np.uint16)
        protect[:, : info["columns"] // 2] = 65535
        mask = ref_image(refmod, protect, "Gray", shim=shim)
        L.SetImageMask.restype = ctypes.c_int
        L.SetImageMask.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        exception = L.AcquireExceptionInfo()
        ok = L.SetImageMask(image.handle, WRITE_PIXEL_MASK, mask.handle, exception)
        L.DestroyExceptionInfo(exception)
        if not ok:
            raise RuntimeError("SetImageMask failed")
    return prepare


def run(px, operator, colorspace="sRGB", mask=None, masked=False):
    """operator(image) -> (image, property or None) on the CPU build and on the HIP-backed one."""
    hdri = px.dtype == np.float32
    cpu_image = ref_image(refmod, px, colorspace, mask=mask)
    gpu_image = ref_image(refmod, px, colorspace, mask=mask, shim=True)
    if masked:
        write_mask(False)(cpu_image)
        write_mask(True)(gpu_image)
    cpu, cpu_property = operator(cpu_image)
    before = calls(hdri)
    gpu, gpu_property = operator(gpu_image)
    got = gpu.numpy()
    return {"accelerated": calls(hdri) - before, "differing": differing(got, cpu.numpy()),
            "changed": differing(np.ascontiguousarray(got[..., :px.shape[2]]), px),
            "gamma": image_gamma(gpu), "cpu_gamma": image_gamma(cpu),
            "property": gpu_property, "cpu_property": cpu_property}


def plain(function, *args):
    return lambda image: (function(image, *args), None)


def linear(black_point, white_point):
    return lambda image: ref_linear_stretch(image, black_point, white_point)


# the library instance the shim loads (one per path): its profile records show which kernels ran
_ = calls(False)
hip = ctypes.CDLL(os.environ["MAGICK_HIP_LIBRARY"])
hip.MhGetPrecision.restype = ctypes.c_int
hip.MhGetProfileRecords.restype = ctypes.c_size_t
hip.MhGetProfileRecords.argtypes = [ctypes.POINTER(Record), ctypes.c_size_t]
hip.MhResetProfileRecords()
hip.MhSetProfileEnabled(1)

Q16, HDRI = np.uint16, np.float32
rgba, rgb_float, gray = gray_pixels(noise(61, 97, 4, Q16)), gray_pixels(noise(61, 97, 3, HDRI)), noise(61, 97, 1, Q16)
narrow = (noise(61, 97, 4, Q16, seed=3) // 3 + 9000)
report = {name: [] for name in ("level", "levelize", "gamma", "negate", "sigmoidal", "linear", "minmax")}
report["level"].append(run(rgba, plain(ref_level, 5000.0, 60000.0, 2.2)))
report["level"].append(run(rgb_float, plain(ref_level, 12345.5, 40000.25, 1.0), "RGB"))
report["level"].append(run(gray, plain(ref_level, 40000.0, 10000.0, 1.7), "Gray"))
report["levelize"].append(run(rgba, plain(ref_levelize, 5000.0, 60000.0, 0.45)))
report["levelize"].append(run(rgb_float, plain(ref_levelize, 3000.0, 50000.0, 1.0), "Lab"))
report["levelize"].append(run(gray, plain(ref_levelize, 5000.0, 60000.0, 2.2), "Gray"))
report["gamma"].append(run(rgba, plain(ref_gamma, 2.2)))
report["gamma"].append(run(rgb_float, plain(ref_gamma, 0.45), "RGB"))
report["gamma"].append(run(gray, plain(ref_gamma, 0.0), "Gray"))
report["negate"].append(run(rgba, plain(ref_negate, False), mask="RGB"))
report["negate"].append(run(rgb_float, plain(ref_negate, True)))
report["negate"].append(run(gray, plain(ref_negate, True), "Gray"))
report["sigmoidal"].append(run(rgba, plain(ref_sigmoidal, 1, 5.0, 32767.5)))
report["sigmoidal"].append(run(rgba, plain(ref_sigmoidal, 0, 5.0, 32767.5), mask="R"))
report["sigmoidal"].append(run(gray, plain(ref_sigmoidal, 1, 10.0, 20000.0), "Gray"))
report["linear"].append(run(rgba, linear(120.0, 60.0)))
report["linear"].append(run(narrow.astype(HDRI), linear(40.0, 20.0), "RGB"))
report["linear"].append(run(gray, linear(20.0, 10.0), "Gray"))
report["minmax"].append(run(narrow, plain(ref_auto_level)))
report["minmax"].append(run(narrow, plain(ref_min_max_stretch, 200.0, 100.0, 2.2), mask="RGB"))
report["minmax"].append(run(np.ascontiguousarray(narrow[..., :1]).astype(HDRI), plain(ref_auto_level), "Gray"))
# GammaImage(1.0) and a contrast below MagickEpsilon return in front of the hook: nothing runs, nothing changes
report["identity"] = [run(rgba, plain(ref_gamma, 1.0)), run(rgba, plain(ref_sigmoidal, 1, 1.0e-13, 32767.5))]
# a write mask the library cannot see: the hook's gate declines
report["masked"] = [run(noise(40, 50, 3, Q16), plain(ref_level, 5000.0, 60000.0, 2.2), masked=True),
                    run(noise(40, 50, 3, Q16), plain(ref_negate, False), masked=True),
                    run(noise(40, 50, 3, Q16) // 3 + 9000, plain(ref_auto_level), masked=True)]

hip.MhSetProfileEnabled(0)
records = (Record * 64)()
n = hip.MhGetProfileRecords(records, 64)
report["kernels"] = sorted({records[i].kernel_name.decode() for i in range(min(n, 64))})
# what mode was that?  (asked LAST; nobody set it)
report["precision"] = int(hip.MhGetPrecision())
print(json.dumps(report))
