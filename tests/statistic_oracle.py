"""StatisticImage on the compiled reference (the oracle has no ref_statistic wrapper: the
MagickCore entry point is called directly), the inputs its rank statistics need, and the
comparison the StatisticImage tests share."""
import ctypes

import numpy as np

# StatisticType, MagickCore/statistic.h:139-152
TYPES = {"Gradient": 1, "Maximum": 2, "Mean": 3, "Median": 4, "Minimum": 5, "Mode": 6, "NonPeak": 7,
         "RootMeanSquare": 8, "StandardDeviation": 9, "Contrast": 10}
RANK = ("Median", "Mode", "NonPeak")
TILE_VIRTUAL_PIXELS = 6          # TileVirtualPixelMethod, cache-view.h:27-46


def _bind(L):
    if getattr(L, "_statistic_bound", False):
        return L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.AcquireExceptionInfo.restype = vp
    L.AcquireExceptionInfo.argtypes = []
    L.DestroyExceptionInfo.restype = vp
    L.DestroyExceptionInfo.argtypes = [vp]
    L.StatisticImage.restype = vp
    L.StatisticImage.argtypes = [vp, ctypes.c_int, sz, sz, vp]
    L.SetImageVirtualPixelMethod.restype = ctypes.c_int
    L.SetImageVirtualPixelMethod.argtypes = [vp, ctypes.c_int, vp]
    L._statistic_bound = True
    return L


def set_virtual_pixels(refmod, image, method):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    L.SetImageVirtualPixelMethod(image.handle, method, exception)
    L.DestroyExceptionInfo(exception)
    return image


def ref_statistic(refmod, image, statistic, width, height):
    """StatisticImage(image, type, width, height) on a refmod.RefImage (either build, the plain
    reference or the HIP-backed MagickCore it was created in); returns a new RefImage."""
    L = _bind(image.L)
    kind = TYPES[statistic] if isinstance(statistic, str) else int(statistic)
    exception = L.AcquireExceptionInfo()
    handle = L.StatisticImage(image.handle, kind, width, height, exception)
    L.DestroyExceptionInfo(exception)
    if not handle:
        raise RuntimeError("StatisticImage failed")
    return refmod.RefImage(handle=handle, lib=L, hdri=image.hdri)


def repeated_keys(rows, cols, channels, dtype, kind, seed=7):
    """Samples with many equal keys, so that mode and nonpeak differ from the minimum and the
    median: "binary" (0 or 65535, 70 % white) or "levels" (five levels, multiples of 16383)."""
    rng = np.random.default_rng(seed)
    if kind == "binary":
        a = (rng.random((rows, cols, channels)) < 0.7).astype(np.uint16) * 65535
    else:
        a = (rng.choice(5, (rows, cols, channels), p=[0.1, 0.35, 0.15, 0.3, 0.1]) * 16383).astype(np.uint16)
    if dtype == np.float32:
        a = a.astype(np.float32)
        if kind == "levels":
            a += np.float32(0.25)              # float keys round to the nearest level: same key
    return np.ascontiguousarray(a)


def assert_same(got, want, what=""):
    """Bit-identical; float NaNs must sit at the same places (their bits may differ)."""
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, got.shape, want.shape)
    if want.dtype == np.uint16:
        bad = got != want
    else:
        nan_got, nan_want = np.isnan(got), np.isnan(want)
        assert np.array_equal(nan_got, nan_want), "%s: NaN at %d places, reference %d" % (
            what, int(nan_got.sum()), int(nan_want.sum()))
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan_want
    if bad.any():
        at = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d of %d samples differ, first at %s: %r != %r" % (
            what, int(bad.sum()), bad.size, at, got[at], want[at]))
