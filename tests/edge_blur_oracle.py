"""BilateralBlurImage and SelectiveBlurImage on the compiled reference (the MagickCore entry points
are called directly, as statistic_oracle.py calls StatisticImage) and the inputs their tests share.

Bilateral inputs stay away from the one table slot the reference never writes
(intensity_gaussian[510]: a tap whose intensity byte is 255 above the centre's): the generators draw
samples from 300 upwards, so no intensity byte is 0."""
import ctypes

import numpy as np


def _bind(L):
    if getattr(L, "_edge_blur_bound", False):
        return L
    vp, sz, dbl, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_char_p
    L.AcquireExceptionInfo.restype = vp
    L.AcquireExceptionInfo.argtypes = []
    L.DestroyExceptionInfo.restype = vp
    L.DestroyExceptionInfo.argtypes = [vp]
    L.BilateralBlurImage.restype = vp
    L.BilateralBlurImage.argtypes = [vp, sz, sz, dbl, dbl, vp]
    L.SelectiveBlurImage.restype = vp
    L.SelectiveBlurImage.argtypes = [vp, dbl, dbl, dbl, vp]
    L.AcquireImageInfo.restype = vp
    L.AcquireImageInfo.argtypes = []
    L.DestroyImageInfo.restype = vp
    L.DestroyImageInfo.argtypes = [vp]
    L.SetImageOption.restype = ctypes.c_int
    L.SetImageOption.argtypes = [vp, cp, cp]
    L.SyncImageSettings.restype = ctypes.c_int
    L.SyncImageSettings.argtypes = [vp, vp, vp]
    L._edge_blur_bound = True
    return L


def _call(refmod, image, name, *args):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    handle = getattr(L, name)(image.handle, *args, exception)
    L.DestroyExceptionInfo(exception)
    if not handle:
        raise RuntimeError("%s failed" % name)
    return refmod.RefImage(handle=handle, lib=L, hdri=image.hdri)


def ref_bilateral(refmod, image, width, height, intensity_sigma, spatial_sigma):
    return _call(refmod, image, "BilateralBlurImage", width, height, intensity_sigma, spatial_sigma)


def ref_selective(refmod, image, radius, sigma, threshold):
    return _call(refmod, image, "SelectiveBlurImage", radius, sigma, threshold)


def set_intensity(image, method):
    """image->intensity, as `-intensity method` sets it: the option of an ImageInfo, synced into
    the image (SyncImageSettings, image.c:4143-4146)."""
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    info = L.AcquireImageInfo()
    ok = L.SetImageOption(info, b"intensity", method.encode()) and L.SyncImageSettings(info, image.handle, exception)
    L.DestroyImageInfo(info)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("intensity method %r rejected" % method)
    return image


def bilateral_pixels(rows, cols, channels, dtype, seed=42, high=65535):
    """Random samples in [300, high]: every intensity byte is at least 1."""
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        f = rng.uniform(300.0, float(high), (rows, cols, channels)).astype(np.float32)
        return np.ascontiguousarray(np.clip(f, np.float32(300.0), np.float32(high)))
    return np.ascontiguousarray(rng.integers(300, min(high, 65535) + 1, (rows, cols, channels), dtype=np.uint16))


def sprite_alpha(px, fraction=0.6, seed=5):
    """The last channel becomes a sprite's alpha: `fraction` of its samples exactly 0."""
    rng = np.random.default_rng(seed)
    out = px.copy()
    out[..., -1][rng.random(px.shape[:2]) < fraction] = 0
    return out
