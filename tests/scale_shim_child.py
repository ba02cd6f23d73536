#!/usr/bin/env python3
"""Child process of tests/test_gpu_scale_shim.py: a FRESH process - no MAGICK_HIP_PRECISION / MAGICKHIP_*
in the environment, no MhSetPrecision call, so the library runs in its default FAST mode - drives
MagickCore's own SampleImage, ScaleImage and ThumbnailImage through the HIP-backed build the way an
unchanged caller does and compares every sample with the plain compiled reference.  The thumbnails are
RGBA frames: ResizeImage keeps the reference's operation order for alpha-weighted channels in either
mode, so every comparison is bit for bit.  Prints one JSON object."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import ref as refmod
from scale_oracle import BIG, EXTREME, THUMBNAILS, _bind, frame, ref_image, ref_sample, ref_scale, ref_thumbnail

for name in list(os.environ):
    if name.startswith("MAGICKHIP_") or name == "MAGICK_HIP_PRECISION":
        del os.environ[name]
os.environ["MAGICK_HIP_LIBRARY"] = os.path.join(ROOT, "imagemagick_amd", "lib", "libmagickhip.so")
READ_PIXEL_MASK, WRITE_PIXEL_MASK, COMPOSITE_PIXEL_MASK = 1, 2, 4      # PixelMask, MagickCore/pixel.h:140-145


class Record(ctypes.Structure):
    _fields_ = [("kernel_name", ctypes.c_char_p), ("count", ctypes.c_ulong), ("min_ms", ctypes.c_double),
                ("max_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


def calls(hdri):
    lib = refmod._load(hdri, True)
    lib.GetMagickHipAcceleratedCalls.restype = ctypes.c_size_t
    return lib.GetMagickHipAcceleratedCalls()


def transfers(hdri):
    lib = refmod._load(hdri, True)
    up, down = ctypes.c_size_t(0), ctypes.c_size_t(0)
    lib.GetMagickHipTransfers(ctypes.byref(up), ctypes.byref(down))
    return up.value, down.value


def differing(got, want):
    if got.shape != want.shape:
        return -1
    return int((got.view(np.uint8) != want.view(np.uint8)).sum())


def set_mask(image, shim, kind):
    """Half of the frame is masked: a channel the library cannot see, the hook's gate declines."""
    L = _bind(image.L)
    info = image.info()
    protect = np.zeros((info["rows"], info["columns"], 1), dtype=np.float32 if image.hdri else np.uint16)
    protect[:, : info["columns"] // 2] = 65535
    mask = ref_image(refmod, protect, "Gray", shim=shim)
    L.SetImageMask.restype = ctypes.c_int
    L.SetImageMask.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    exception = L.AcquireExceptionInfo()
    ok = L.SetImageMask(image.handle, kind, mask.handle, exception)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("SetImageMask failed")


def run(px, operator, colorspace="sRGB", mask=None, masked=0):
    """operator(refmod, image) on the CPU build and on the HIP-backed one."""
    hdri = px.dtype == np.float32
    cpu_image = ref_image(refmod, px, colorspace, mask=mask)
    gpu_image = ref_image(refmod, px, colorspace, mask=mask, shim=True)
    if masked:
        set_mask(cpu_image, False, masked)
        set_mask(gpu_image, True, masked)
    cpu = operator(refmod, cpu_image)
    before, moved = calls(hdri), transfers(hdri)
    gpu = operator(refmod, gpu_image)
    accelerated, computed = calls(hdri) - before, transfers(hdri)
    got = gpu.numpy()
    delivered = transfers(hdri)
    return {"accelerated": accelerated, "differing": differing(got, cpu.numpy()),
            "type": gpu.info()["type"], "cpu_type": cpu.info()["type"],
            "uploads": computed[0] - moved[0], "downloads_before_the_read": computed[1] - moved[1],
            "downloads": delivered[1] - moved[1], "uploads_after_the_read": delivered[0] - moved[0]}


def sample(rows, cols, offset=None):
    return lambda refmod, image: ref_sample(refmod, image, rows, cols, offset)


def scale(rows, cols):
    return lambda refmod, image: ref_scale(refmod, image, rows, cols)


def thumbnail(rows, cols):
    return lambda refmod, image: ref_thumbnail(refmod, image, rows, cols)


# the library instance the shim loads (one per path): its profile records show which kernels ran
_ = calls(False)
hip = ctypes.CDLL(os.environ["MAGICK_HIP_LIBRARY"])
hip.MhGetPrecision.restype = ctypes.c_int
hip.MhGetProfileRecords.restype = ctypes.c_size_t
hip.MhGetProfileRecords.argtypes = [ctypes.POINTER(Record), ctypes.c_size_t]
hip.MhResetProfileRecords()
hip.MhSetProfileEnabled(1)

Q16, HDRI = np.uint16, np.float32
report = {name: [] for name in ("sample", "scale", "thumbnail")}
rgba = frame("rgba", 61, 97, Q16, seed=1, transparent=0.3)
rgb_float = frame("rgb", 53, 37, HDRI, seed=2)
gray = frame("gray", 64, 64, Q16, seed=3)
report["sample"].append(run(rgba, sample(130, 20)))
report["sample"].append(run(rgb_float, sample(7, 11, "25x75"), "RGB"))
report["sample"].append(run(gray, sample(16, 16, "100"), "Gray"))
report["scale"].append(run(rgba, scale(130, 20)))
report["scale"].append(run(rgb_float, scale(7, 11), "RGB"))
report["scale"].append(run(gray, scale(16, 16), "Gray"))
report["scale"].append(run(frame("rgba", BIG[0][0], BIG[0][1], HDRI, seed=4, transparent=0.3), scale(*BIG[1])))
report["scale"].append(run(frame("rgba", EXTREME[0][0], EXTREME[0][1], Q16, seed=5), scale(*EXTREME[1]), mask="RGB"))
for index, ((rows, cols), (to_rows, to_cols)) in enumerate(THUMBNAILS):
    for dtype in (Q16, HDRI):
        case = run(frame("rgba", rows, cols, dtype, seed=6 + index, transparent=0.3), thumbnail(to_rows, to_cols))
        case["stages"] = (1 if cols // to_cols > 4 and rows // to_rows > 4 else 0) + \
            (1 if cols // to_cols > 2 and rows // to_rows > 2 else 0) + 1
        report["thumbnail"].append(case)
# same-size requests return in front of the hooks
report["identity"] = [run(rgba, sample(61, 97)), run(rgba, scale(61, 97))]
# a sample:offset whose rows are virtual pixels, and a colourspace outside the gate: the hook declines
report["declined"] = [run(rgba, sample(130, 20, "50x150")), run(rgba, sample(130, 20, "0x101")),
                      run(rgba, sample(130, 20), "Lab"), run(rgba, scale(130, 20), "Lab")]
# ... and a mask, which the library cannot see.  A read mask: neither operator consults it, the mask channel
# is copied or scaled like any other, and the CPU result is reproducible: compared sample by sample
masked_frame = frame("rgb", 40, 50, Q16, seed=7)
masked_float = frame("rgba", 40, 50, HDRI, seed=8, transparent=0.3)
report["masked"] = [run(px, operator, masked=READ_PIXEL_MASK) for px in (masked_frame, masked_float)
                    for operator in (sample(13, 31), scale(13, 31), scale(90, 20))]
# A write or a composite mask: the reference sizes the result with CloneImage, which leaves the new pixel
# cache - the mask channel included - unset.  Both operators skip the pixels whose (unset) write mask protects
# them (resize.c:4031, :4380, :4477), and the cache blends what they store with the unset pixels by the (unset)
# composite mask when a row is synced: the reference's own two runs differ, so only the path and the geometry
# are compared
report["unset_masked"] = [run(masked_frame, operator, masked=kind) for kind in (WRITE_PIXEL_MASK, COMPOSITE_PIXEL_MASK)
                          for operator in (sample(13, 31), scale(13, 31))]

hip.MhSetProfileEnabled(0)
records = (Record * 64)()
n = hip.MhGetProfileRecords(records, 64)
report["kernels"] = sorted({records[i].kernel_name.decode() for i in range(min(n, 64))})
# what mode was that?  (asked LAST; nobody set it)
report["precision"] = int(hip.MhGetPrecision())
print(json.dumps(report))
