"""The threshold operators of MagickCore/threshold.c on the compiled reference (the entry points are
called directly, as kuwahara_oracle.py calls KuwaharaImage), the layouts and inputs their tests share,
and a NumPy restatement of all six (the float chain of AdaptiveThresholdImage included) that
tests/test_threshold_model.py holds against the compiled reference bit for bit."""
import ctypes

import numpy as np

from kuwahara_oracle import (noise, constant, flat_blocks, step_edge, wide_range_float,  # noqa: F401
                             out_of_range_float)

QR = 65535.0
EPSILON = 1.0e-12
SHAPES = [(1, 1), (1, 40), (40, 1), (15, 17), (61, 97), (130, 70)]          # rows x columns
LAYOUTS = ["gray", "gray+alpha", "rgb", "rgba", "plain4"]
CHANNELS = {"gray": 1, "gray+alpha": 2, "rgb": 3, "rgba": 4, "plain4": 4}
METHODS = {"Kapur": 1, "OTSU": 2, "Triangle": 3}                              # threshold.h:25-31
INTENSITIES = {"Average": 1, "Brightness": 2, "Lightness": 3, "MS": 4, "Rec601Luma": 5, "Rec601Luminance": 6,
               "Rec709Luma": 7, "Rec709Luminance": 8, "RMS": 9}
# ChannelType bits (pixel.h:60-75) and the stored offsets left out, per mask name, of an RGBA frame
MASKS = {"R": (0x1, (1, 2, 3)), "RGB": (0x7, (3,)), "A": (0x10, (0, 1, 2))}


def _bind(L):
    if getattr(L, "_threshold_bound", False):
        return L
    vp, sz, dbl, cp, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_char_p, ctypes.c_int
    L.AcquireExceptionInfo.restype = vp
    L.AcquireExceptionInfo.argtypes = []
    L.DestroyExceptionInfo.restype = vp
    L.DestroyExceptionInfo.argtypes = [vp]
    L.AdaptiveThresholdImage.restype = vp
    L.AdaptiveThresholdImage.argtypes = [vp, sz, sz, dbl, vp]
    L.AutoThresholdImage.restype = i
    L.AutoThresholdImage.argtypes = [vp, i, vp]
    L.BilevelImage.restype = i
    L.BilevelImage.argtypes = [vp, dbl, vp]
    L.BlackThresholdImage.restype = i
    L.BlackThresholdImage.argtypes = [vp, cp, vp]
    L.WhiteThresholdImage.restype = i
    L.WhiteThresholdImage.argtypes = [vp, cp, vp]
    L.RangeThresholdImage.restype = i
    L.RangeThresholdImage.argtypes = [vp, dbl, dbl, dbl, dbl, vp]
    L.GetImageProperty.restype = cp
    L.GetImageProperty.argtypes = [vp, cp, vp]
    L.AcquireImageInfo.restype = vp
    L.AcquireImageInfo.argtypes = []
    L.DestroyImageInfo.restype = vp
    L.DestroyImageInfo.argtypes = [vp]
    L.SetImageOption.restype = i
    L.SetImageOption.argtypes = [vp, cp, cp]
    L.SyncImageSettings.restype = i
    L.SyncImageSettings.argtypes = [vp, vp, vp]
    L._threshold_bound = True
    return L


def _in_place(image, name, *args):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    ok = getattr(L, name)(image.handle, *args, exception)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("%s failed" % name)
    return image


def ref_bilevel(image, threshold):
    return _in_place(image, "BilevelImage", float(threshold))


def ref_auto_threshold(image, method):
    """AutoThresholdImage in place; returns (image, the auto-threshold:threshold property string)."""
    _in_place(image, "AutoThresholdImage", METHODS[method] if isinstance(method, str) else int(method))
    return image, get_property(image, "auto-threshold:threshold")


def get_property(image, key):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    value = L.GetImageProperty(image.handle, key.encode(), exception)
    L.DestroyExceptionInfo(exception)
    return None if value is None else value.decode()


def _geometry(thresholds):
    """Per-channel thresholds in Quantum units as the reference's geometry string: red, green, blue,
    alpha (threshold.c:964-975)."""
    return ",".join("%.17g" % float(t) for t in thresholds).encode()


def ref_black_threshold(image, thresholds):
    return _in_place(image, "BlackThresholdImage", _geometry(thresholds))


def ref_white_threshold(image, thresholds):
    return _in_place(image, "WhiteThresholdImage", _geometry(thresholds))


def ref_range_threshold(image, low_black, low_white, high_white, high_black):
    return _in_place(image, "RangeThresholdImage", float(low_black), float(low_white), float(high_white),
                     float(high_black))


def ref_adaptive_threshold(refmod, image, width, height, bias):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    handle = L.AdaptiveThresholdImage(image.handle, int(width), int(height), float(bias), exception)
    L.DestroyExceptionInfo(exception)
    if not handle:
        raise RuntimeError("AdaptiveThresholdImage failed")
    return refmod.RefImage(handle=handle, lib=L, hdri=image.hdri)


def set_intensity(image, method):
    """image->intensity, as `-intensity method` sets it (SyncImageSettings, image.c)."""
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    info = L.AcquireImageInfo()
    ok = L.SetImageOption(info, b"intensity", method.encode()) and L.SyncImageSettings(info, image.handle, exception)
    L.DestroyImageInfo(info)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("intensity method %r rejected" % method)
    return image


def ref_image(refmod, px, colorspace="sRGB", mask=None, intensity=None, shim=False):
    """px in the reference's pixel cache.  Four plain channels go in as R,G,B,A: under the default
    channel mask the reference treats alpha like any other channel in all six operators."""
    image = refmod.RefImage(px, colorspace, shim=shim)
    if mask is not None:
        image.set_channel_mask(mask)
    if intensity is not None:
        set_intensity(image, intensity)
    return image


def kept_channels_equal(got, px, kept):
    """The stored offsets `kept` of got carry the bits of px."""
    kept = list(kept)
    return np.array_equal(np.ascontiguousarray(got[..., kept]).view(np.uint8),
                          np.ascontiguousarray(px[..., kept]).view(np.uint8))


def frame(layout, rows, cols, dtype, seed=0):
    return noise(rows, cols, CHANNELS[layout], dtype, seed=1775 + seed)


def two_level(rows, cols, channels, dtype, low=12000, high=47000, seed=2):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.where(rng.random((rows, cols, 1)) < 0.35, low, high).repeat(channels, 2).astype(dtype))


def frame_with_histogram(counts):
    """A one-channel Q16 frame (1 x N) whose AutoThresholdImage histogram is `counts`: bin b holds the
    samples 257*b."""
    values = np.repeat(np.arange(256, dtype=np.int64) * 257, np.asarray(counts, dtype=np.int64))
    return np.ascontiguousarray(values.astype(np.uint16).reshape(1, -1, 1))


# -------------------------------------------------------------------------------------- restatement
def _clamp(values, dtype):
    """ClampToQuantum, quantum.h:86-97."""
    if dtype == np.float32:
        return values.astype(np.float32)
    out = np.floor(np.clip(values, 0.0, QR) + 0.5)
    out[~(values > 0.0)] = 0.0
    out[values >= QR] = QR
    return out.astype(np.uint16)


def _perceptible_reciprocal(x):
    sign = -1.0 if x < 0.0 else 1.0
    return 1.0 / x if sign * x >= EPSILON else sign / EPSILON


def intensity(px):
    """GetPixelIntensity with the default method on a gray or sRGB frame (pixel.c:2356-2455)."""
    p = px.astype(np.float64)
    if px.shape[2] == 1:
        return p[..., 0]
    if px.shape[2] == 2:
        return 0.212656 * p[..., 0] + 0.715158 * p[..., 0] + 0.072186 * p[..., 0]
    return 0.212656 * p[..., 0] + 0.715158 * p[..., 1] + 0.072186 * p[..., 2]


def restate_pointwise(px, mode, update, per_channel, thresholds=None, range_points=None):
    """Bilevel / Black / White / Range.  update: the stored offsets written; per_channel: the channel
    mask is not AllChannels."""
    dtype = px.dtype.type
    out = px.copy()
    whole = intensity(px)
    for c in update:
        pixel = px[..., c].astype(np.float64) if per_channel else whole
        q = px[..., c]
        if mode == "bilevel":
            out[..., c] = np.where(pixel <= thresholds[0], 0, 65535).astype(dtype)
        elif mode == "black":
            out[..., c] = np.where(pixel < thresholds[c], dtype(0), q)
        elif mode == "white":
            out[..., c] = np.where(pixel > thresholds[c], dtype(65535), q)
        else:
            low_black, low_white, high_white, high_black = range_points
            rising = _clamp(QR * _perceptible_reciprocal(low_white - low_black) * (pixel - low_black), dtype)
            falling = _clamp(QR * _perceptible_reciprocal(high_black - high_white) * (high_black - pixel), dtype)
            value = np.zeros(pixel.shape, dtype=dtype)
            value = np.where((pixel > high_white) & (pixel <= high_black), falling, value)
            value = np.where((pixel >= low_white) & (pixel <= high_white), dtype(65535), value)
            value = np.where((pixel >= low_black) & (pixel < low_white), rising, value)
            value = np.where(pixel < low_black, dtype(0), value)
            out[..., c] = value
    return out


def histogram(px):
    """256 counts of ScaleQuantumToChar(ClampToQuantum(intensity)), quantum.h:113-124."""
    value = intensity(px)
    if px.dtype == np.float32:
        q = value.astype(np.float32)
        with np.errstate(invalid="ignore"):
            scaled = q / np.float32(257.0)
            bins = np.where(~(q > 0), 0, np.where(scaled >= np.float32(255.0), 255,
                            (np.minimum(scaled, np.float32(255.0)) + np.float32(0.5)).astype(np.int64)))
    else:
        q = _clamp(value, np.uint16).astype(np.int64)
        bins = ((q + 128) - ((q + 128) >> 8)) >> 8
    return np.bincount(bins.ravel().astype(np.int64), minlength=256).astype(np.float64)


def restate_adaptive(px, width, height, bias, copy=()):
    """threshold.c:239-337 statement for statement: the running fp64 sum of every (row, channel)
    from column 0 to the end of the row."""
    rows, cols, channels = px.shape
    dtype = px.dtype.type
    if width == 0 or height == 0:
        return px.copy()
    out = px.copy()
    ys = np.clip(np.arange(rows)[:, None] - height // 2 + np.arange(height)[None, :], 0, rows - 1)   # [row, v]
    number_pixels = float(width * height)
    for c in range(channels):
        if c in copy:
            continue
        plane = px[..., c].astype(np.float64)
        channel_bias = np.zeros(rows)
        channel_sum = np.zeros(rows)
        for v in range(height):
            for u in range(width):
                sample = plane[ys[:, v], min(max(u - width // 2, 0), cols - 1)]
                if u == width - 1:
                    channel_bias = channel_bias + sample
                channel_sum = channel_sum + sample
        for x in range(cols):
            channel_sum = channel_sum - channel_bias
            channel_bias = np.zeros(rows)
            first = min(max(x - width // 2, 0), cols - 1)
            last = min(max(x - width // 2 + width - 1, 0), cols - 1)
            for v in range(height):
                channel_bias = channel_bias + plane[ys[:, v], first]
                channel_sum = channel_sum + plane[ys[:, v], last]
            mean = channel_sum / number_pixels + bias
            out[:, x, c] = np.where(plane[:, x] <= mean, 0, 65535).astype(dtype)
    return out
