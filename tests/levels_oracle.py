"""The level operators of MagickCore/enhance.c and histogram.c on the compiled reference (the exported
entry points are called directly, as threshold_oracle.py does), the inputs their tests share, and a
NumPy restatement of all of them that tests/test_levels_model.py holds against the compiled reference
bit for bit.  pow, tanh and atanh are the C library's, through `math`, one call per distinct sample."""
import ctypes
import math

import numpy as np

from kuwahara_oracle import noise, constant, out_of_range_float  # noqa: F401
from threshold_oracle import (CHANNELS, MASKS, ref_image, get_property, kept_channels_equal, intensity,  # noqa: F401
                              _bind as _bind_threshold)

QR = 65535.0
QS = 1.0 / 65535.0
EPSILON = 1.0e-12
MAXIMUM_VALUE = 1.79769313486231570E+308           # MagickMaximumValue, magick-type.h:115
MINIMUM_VALUE = 2.22507385850720140E-308           # MagickMinimumValue
LAYOUTS = ["gray", "gray+alpha", "rgb", "rgba"]
# (black, white, gamma): the sets checked against the reference table by table, white == black,
# white < black, and gamma in {0, 0.45, 1, 2.2}
LEVELS = [(5000.0, 60000.0, 2.2), (0.0, 65535.0, 0.45), (12345.5, 40000.25, 1.0), (40000.0, 10000.0, 1.7),
          (30000.0, 30000.0, 1.0), (30000.0, 30000.0, 2.2), (1000.0, 50000.0, 0.0), (-2000.5, 70000.0, 1.0)]
# (sharpen, contrast, midpoint): the checked sets, midpoints 0 and QuantumRange, a contrast below MagickEpsilon
SIGMOIDALS = [(1, 5.0, 32767.5), (0, 5.0, 32767.5), (1, 10.0, 20000.0), (0, 3.0, 0.0), (1, 3.0, 0.0),
              (1, 7.0, QR), (0, 7.0, QR), (1, 1.0e-13, 32767.5), (0, 0.0, 32767.5)]
GAMMAS = [2.2, 0.45, 1.0, 0.0, 1.7]


def _bind(L):
    _bind_threshold(L)
    if getattr(L, "_levels_bound", False):
        return L
    vp, dbl, i = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    for name, extra in (("LevelImage", [dbl, dbl, dbl]), ("LevelizeImage", [dbl, dbl, dbl]), ("GammaImage", [dbl]),
                        ("NegateImage", [i]), ("SigmoidalContrastImage", [i, dbl, dbl]),
                        ("MinMaxStretchImage", [dbl, dbl, dbl]), ("AutoLevelImage", []),
                        ("LinearStretchImage", [dbl, dbl]), ("NormalizeImage", []),
                        ("BrightnessContrastImage", [dbl, dbl])):
        fn = getattr(L, name)
        fn.restype = i
        fn.argtypes = [vp] + extra + [vp]
    L.GetImageRange.restype = i
    L.GetImageRange.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl), vp]
    L._levels_bound = True
    return L


def _in_place(image, name, *args):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    ok = getattr(L, name)(image.handle, *args, exception)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("%s failed" % name)
    return image


def ref_level(image, black, white, gamma):
    return _in_place(image, "LevelImage", float(black), float(white), float(gamma))


def ref_levelize(image, black, white, gamma):
    return _in_place(image, "LevelizeImage", float(black), float(white), float(gamma))


def ref_gamma(image, gamma):
    return _in_place(image, "GammaImage", float(gamma))


def ref_negate(image, grayscale):
    return _in_place(image, "NegateImage", 1 if grayscale else 0)


def ref_sigmoidal(image, sharpen, contrast, midpoint):
    return _in_place(image, "SigmoidalContrastImage", 1 if sharpen else 0, float(contrast), float(midpoint))


def ref_min_max_stretch(image, black, white, gamma):
    return _in_place(image, "MinMaxStretchImage", float(black), float(white), float(gamma))


def ref_auto_level(image):
    return _in_place(image, "AutoLevelImage")


def ref_linear_stretch(image, black_point, white_point):
    """LinearStretchImage in place; returns (image, the histogram:linear-stretch property string)."""
    _in_place(image, "LinearStretchImage", float(black_point), float(white_point))
    return image, get_property(image, "histogram:linear-stretch")


def ref_normalize(image):
    return _in_place(image, "NormalizeImage")


def ref_brightness_contrast(image, brightness, contrast):
    return _in_place(image, "BrightnessContrastImage", float(brightness), float(contrast))


def ref_range(image):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    minimum, maximum = ctypes.c_double(0.0), ctypes.c_double(0.0)
    L.GetImageRange(image.handle, ctypes.byref(minimum), ctypes.byref(maximum), exception)
    L.DestroyExceptionInfo(exception)
    return minimum.value, maximum.value


def linear_stretch_property(black, white):
    """enhance.c:3423-3424."""
    return "%gx%g%%" % (100.0 * black / 65535, 100.0 * white / 65535)


# ------------------------------------------------------------------------------------------ inputs
def ramp(channels, dtype):
    """All 65536 Q16 values as 256 x 256 x channels; channel c walks the ramp from another start."""
    base = np.arange(65536, dtype=np.int64).reshape(256, 256, 1)
    px = (base + np.arange(channels).reshape(1, 1, -1) * 21845) % 65536
    return np.ascontiguousarray(px.astype(dtype))


def frame(layout, rows, cols, dtype, seed=0):
    return noise(rows, cols, CHANNELS[layout], dtype, seed=2913 + seed)


def gray_pixels(px, fraction=0.4, seed=6):
    """`fraction` of the pixels of an RGB[A] frame get R == G == B (NegateImage with grayscale)."""
    rng = np.random.default_rng(seed)
    out = px.copy()
    gray = rng.random(px.shape[:2]) < fraction
    out[gray, 1] = out[gray, 0]
    out[gray, 2] = out[gray, 0]
    return out


def seed_frame(dtype):
    """The frame of the issue's second property: 8 x 8 RGB, channels 1 and 2 in [20000, 40000),
    channel 0's minimum and maximum both in column 0."""
    rng = np.random.default_rng(11)
    px = rng.integers(20000, 40000, (8, 8, 3)).astype(dtype)
    px[..., 0] = rng.integers(25000, 35000, (8, 8)).astype(dtype)
    px[2, 0, 0] = 3000
    px[5, 0, 0] = 61000
    return np.ascontiguousarray(px)


# -------------------------------------------------------------------------------------- restatement
def _clamp(values, dtype):
    """ClampToQuantum, quantum.h:86-97."""
    values = np.asarray(values, dtype=np.float64)
    if dtype == np.float32:
        with np.errstate(over="ignore"):
            return values.astype(np.float32)
    out = np.floor(np.clip(values, 0.0, QR) + 0.5)
    out[~(values > 0.0)] = 0.0
    out[values >= QR] = QR
    return out.astype(np.uint16)


def _clamp_pixel(values):
    """ClampPixel on a stored float (ClampImage, threshold.c:1163)."""
    out = values.copy()
    out[values.astype(np.float64) < 0.0] = np.float32(0.0)
    out[values.astype(np.float64) >= QR] = np.float32(QR)
    return out


def _perceptible_reciprocal(x):
    sign = -1.0 if x < 0.0 else 1.0
    return 1.0 / x if sign * x >= EPSILON else sign / EPSILON


def _pow(x, y):
    """The C library's pow: math.pow raises where C returns infinity."""
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.inf if x == 0.0 else math.nan


def _gamma_pow(value, gamma):
    return value if value < 0.0 else _pow(value, gamma)


def _per_sample(fn, plane):
    """fn (a scalar double -> double) over a plane, one call per distinct sample."""
    values, inverse = np.unique(plane, return_inverse=True)
    mapped = np.array([fn(float(v)) for v in values], dtype=np.float64)
    return mapped[inverse].reshape(plane.shape)


def level(px, update, black, white, gamma):
    dtype = px.dtype.type
    scale = _perceptible_reciprocal(white - black)
    exponent = _perceptible_reciprocal(gamma)
    out = px.copy()
    for c in update:
        value = _clamp(_per_sample(lambda q: QR * _gamma_pow(scale * (q - black), exponent), px[..., c]), dtype)
        out[..., c] = _clamp_pixel(value) if dtype == np.float32 else value
    return out


def levelize(px, update, black, white, gamma):
    dtype = px.dtype.type
    out = px.copy()
    for c in update:
        out[..., c] = _clamp(_per_sample(lambda q: _gamma_pow(QS * q, gamma) * (white - black) + black, px[..., c]), dtype)
    return out


def scale_map_to_quantum(value, dtype):
    if value <= 0.0:
        return 0.0
    if value >= 65535:
        return QR
    return float(int(value + 0.5)) if dtype == np.uint16 else float(np.float32(value))


def scale_quantum_to_map(values, dtype):
    """ScaleQuantumToMap of Quantum-typed samples, quantum-private.h:504-515."""
    if dtype == np.uint16:
        return values.astype(np.int64)
    with np.errstate(invalid="ignore"):
        q = values.astype(np.float32)
        return np.where(q >= np.float32(65535.0), 65535,
                        np.where(~(q > 0), 0, (np.minimum(q, np.float32(65535.0)) + np.float32(0.5)).astype(np.int64)))


def gamma_map(gamma, dtype):
    """GammaImage's map, enhance.c:2354-2362."""
    table = np.zeros(65536, dtype=np.float64)
    if gamma != 0.0:
        exponent = _perceptible_reciprocal(gamma)
        for i in range(65536):
            table[i] = scale_map_to_quantum(65535 * _pow(i / 65535, exponent), dtype)
    return table


def gamma(px, update, value):
    if value == 1.0:
        return px.copy()
    dtype = px.dtype.type
    table = gamma_map(value, dtype).astype(dtype)
    out = px.copy()
    for c in update:
        out[..., c] = table[scale_quantum_to_map(_clamp(px[..., c].astype(np.float64), dtype), dtype)]
    return out


def negate(px, update, grayscale):
    out = px.copy()
    touched = np.ones(px.shape[:2], dtype=bool)
    colours = px.shape[2] - (1 if px.shape[2] in (2, 4) else 0)
    if grayscale and colours >= 3:
        p = px.astype(np.float64)
        touched = (np.abs(p[..., 0] - p[..., 1]) < EPSILON) & (np.abs(p[..., 1] - p[..., 2]) < EPSILON)
    for c in update:
        value = (np.float32(65535.0) - px[..., c]) if px.dtype == np.float32 else (65535 - px[..., c].astype(np.int64))
        out[..., c] = np.where(touched, value.astype(px.dtype), px[..., c])
    return out


def sigmoidal(px, update, sharpen, contrast, midpoint):
    if contrast < EPSILON:
        return px.copy()
    dtype = px.dtype.type
    a, b = contrast, QS * midpoint

    def sig(x):
        return math.tanh((0.5 * a) * (x - b))

    sig0, sig1 = sig(0.0), sig(1.0)

    def forward(q):
        return QR * ((sig(QS * q) - sig0) / (sig1 - sig0))

    def inverse(q):
        argument = (sig1 - sig0) * (QS * q) + sig0
        clamped = -1 + EPSILON if argument < -1 + EPSILON else (1 - EPSILON if argument > 1 - EPSILON else argument)
        return QR * (b + (2.0 / a) * math.atanh(clamped))

    out = px.copy()
    for c in update:
        out[..., c] = _clamp(_per_sample(forward if sharpen else inverse, px[..., c]), dtype)
    return out


def image_range(px, update):
    """GetImageRange, statistic.c:1851-1929: every row is seeded with the offset-0 sample of its
    first pixel, whatever the mask."""
    minimum, maximum = MAXIMUM_VALUE, MINIMUM_VALUE
    if px.shape[0] == 0 or px.shape[1] == 0:
        return minimum, maximum
    planes = [px[:, 0, 0].astype(np.float64)] + [px[..., c].astype(np.float64) for c in update]
    for plane in planes:
        minimum = min(minimum, float(plane.min()))
        maximum = max(maximum, float(plane.max()))
    return minimum, maximum


def min_max_stretch(px, update, all_channels, black, white, value, alpha_offset=None):
    """MinMaxStretchImage, histogram.c:927-975.  update: the stored offsets whose trait carries
    Update; all_channels: the mask is AllChannels.  Otherwise offset i is selected with the
    ChannelType bit 1 << i, which names no stored channel at the alpha offset."""
    if alpha_offset is None:
        alpha_offset = px.shape[2] - 1 if px.shape[2] in (2, 4) else -1
    if all_channels:
        minimum, maximum = image_range(px, update)
        minimum += black
        maximum -= white
        return level(px, update, minimum, maximum, value) if abs(minimum - maximum) >= EPSILON else px.copy()
    out = px.copy()
    for i in update:
        selected = () if i == alpha_offset else (i,)
        minimum, maximum = image_range(out, selected)
        minimum += black
        maximum -= white
        if abs(minimum - maximum) >= EPSILON:
            out = level(out, selected, minimum, maximum, value)
    return out


def linear_stretch(px, update, black_point, white_point):
    """LinearStretchImage, enhance.c:3347-3427 -> (pixels, black, white)."""
    dtype = px.dtype.type
    bins = scale_quantum_to_map(_clamp(intensity(px), dtype), dtype)
    counts = np.bincount(bins.ravel().astype(np.int64), minlength=65536).astype(np.float64)
    total, black = 0.0, 0
    while black < 65535:
        total += counts[black]
        if total >= black_point:
            break
        black += 1
    total, white = 0.0, 65535
    while white != 0:
        total += counts[white]
        if total >= white_point:
            break
        white -= 1
    out = level(px, update, scale_map_to_quantum(float(black), dtype), scale_map_to_quantum(float(white), dtype), 1.0)
    return out, black, white


def brightness_contrast_coefficients(brightness, contrast):
    """enhance.c:244-249: FunctionImage(Polynomial) with these two."""
    slope = 100.0 * _perceptible_reciprocal(100.0 - contrast)
    if contrast < 0.0:
        slope = 0.01 * contrast + 1.0
    return [slope, (0.01 * brightness - 0.5) * slope + 0.5]


def polynomial(px, update, coefficients):
    """ApplyFunction(Polynomial), statistic.c:1031-1041."""
    dtype = px.dtype.type
    out = px.copy()
    for c in update:
        pixel = px[..., c].astype(np.float64)
        result = np.zeros(pixel.shape)
        for k in coefficients:
            result = result * QS * pixel + k
        out[..., c] = _clamp(QR * result, dtype)
    return out
