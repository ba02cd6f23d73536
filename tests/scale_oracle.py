"""SampleImage, ScaleImage and ThumbnailImage of MagickCore/resize.c on the compiled reference (the entry
points are called directly, as threshold_oracle.py calls its operators), the geometries and frames their
tests share, and a NumPy restatement of SampleImage and ScaleImage built on Python plans: the two state
machines of ScaleImage restated statement for statement, turned into ordered (source, weight) term lists.
tests/test_scale_model.py holds the restatement against the compiled reference bit for bit, and the
library's host plan (MhScaleImagePlan) against the Python plan term for term."""
import ctypes

import numpy as np

from kuwahara_oracle import noise, out_of_range_float  # noqa: F401
from threshold_oracle import MASKS, ref_image  # noqa: F401

QR = 65535.0
QS = 1.0 / 65535.0
EPSILON = 1.0e-12
LAYOUTS = ["gray", "gray+alpha", "rgb", "rgba"]
CHANNELS = {"gray": 1, "gray+alpha": 2, "rgb": 3, "rgba": 4}

# (source rows, columns) -> (destination rows, columns): the smallest that reach each branch
BIG = ((300, 700), (131, 333))         # the one-launch kernel works on runs of 256 destination columns, one
#                                        destination row each, 256 lanes: two runs, three trips over the staged
#                                        source interval of the first (538 columns), many rows
EXTREME = ((3, 2000), (3, 3))          # column term lists of about 670: the generic two-launch form
FUSED = ((64, 64), (16, 16))
# The one-launch kernel stages the source interval of a run as [columns][channels] doubles in at most 64 KiB and
# halves the run (256, 128, 64, 32 destination columns) until it fits.  RGBA: 2048 columns are the limit.
LIMIT = ((2, 2048), (2, 256))          # one run of 256 whose interval is all 2048 columns: 64 KiB exactly
HALVED = ((2, 4200), (2, 420))         # a run of 256 reads 2561 columns (80 KiB): runs of 128, four of them
GEOMETRIES = [((53, 37), (7, 11)),     # non-integer reduction
              FUSED,                   # integer reduction
              ((16, 16), (64, 64)), ((37, 53), (80, 90)),        # enlargements
              ((64, 64), (63, 65)),    # near identity, one axis each way
              ((40, 31), (40, 9)), ((40, 31), (13, 31)),         # equal rows, equal columns
              ((1, 1), (5, 3)), ((40, 1), (1, 1)), ((1, 40), (3, 1)),
              ((61, 97), (130, 20)),   # reduce one axis, enlarge the other
              BIG, EXTREME, LIMIT, HALVED]
SAMPLE_OFFSETS = [None, "0", "25x75", "100"]          # the sample:offset artifact
THUMBNAILS = [((600, 500), (100, 83)),   # rows x columns; factors 6 and 6: sample, Box, final
              ((300, 300), (100, 100)),  # factor 3: Box, final
              ((150, 150), (100, 100))]  # factor 1: final only


def layout_has_alpha(layout):
    return layout in ("gray+alpha", "rgba")


def frame(layout, rows, cols, dtype, seed=0, transparent=0.0):
    """Noise over the whole range; `transparent`: that share of the alpha samples exactly 0."""
    px = noise(rows, cols, CHANNELS[layout], dtype, seed=4106 + seed)
    if transparent > 0.0 and layout_has_alpha(layout):
        rng = np.random.default_rng(seed + 17)
        px[..., -1][rng.random((rows, cols)) < transparent] = 0
    return px


def negative_alpha_float(rows, cols, channels, seed=6):
    """Float samples whose alpha runs from -QuantumRange to QuantumRange: both branches of
    PerceptibleReciprocal, and scaled alphas that cancel to almost nothing."""
    rng = np.random.default_rng(seed)
    px = rng.uniform(-20000.0, 90000.0, (rows, cols, channels)).astype(np.float32)
    px[..., -1] = rng.uniform(-65535.0, 65535.0, (rows, cols)).astype(np.float32)
    px[..., -1][rng.random((rows, cols)) < 0.2] = 0.0
    return np.ascontiguousarray(px)


# ------------------------------------------------------------------------------- compiled reference
def _bind(L):
    if getattr(L, "_scale_bound", False):
        return L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.AcquireExceptionInfo.restype = vp
    L.AcquireExceptionInfo.argtypes = []
    L.DestroyExceptionInfo.restype = vp
    L.DestroyExceptionInfo.argtypes = [vp]
    for name in ("SampleImage", "ScaleImage", "ThumbnailImage"):
        fn = getattr(L, name)
        fn.restype = vp
        fn.argtypes = [vp, sz, sz, vp]
    L._scale_bound = True
    return L


def _new_image(refmod, image, name, columns, rows):
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    handle = getattr(L, name)(image.handle, int(columns), int(rows), exception)
    L.DestroyExceptionInfo(exception)
    if not handle:
        raise RuntimeError("%s failed" % name)
    return refmod.RefImage(handle=handle, lib=L, hdri=image.hdri)


def ref_sample(refmod, image, rows, columns, offset=None):
    """offset: the sample:offset artifact string, None = unset."""
    if offset is not None:
        image.set_artifact("sample:offset", offset)
    return _new_image(refmod, image, "SampleImage", columns, rows)


def ref_scale(refmod, image, rows, columns):
    return _new_image(refmod, image, "ScaleImage", columns, rows)


def ref_thumbnail(refmod, image, rows, columns):
    return _new_image(refmod, image, "ThumbnailImage", columns, rows)


def offset_percent(offset):
    """The artifact string as the (x, y) percentages of the C ABI (ParseGeometry: rho[xsigma])."""
    if offset is None:
        return (-1.0, -1.0)
    parts = offset.split("x")
    return (float(parts[0]), float(parts[1] if len(parts) > 1 else parts[0]))


# ------------------------------------------------------------------------------------ Python plans
def plan_rows(source, destination):
    """resize.c:4196-4199, :4262-4372.  Per destination row the ordered [(source row, weight)] terms:
    the y_vector accumulations, then the span.y term.  None on the equal-rows path."""
    if source == destination:
        return None
    plan = []
    number_rows, next_row, span, row = 0, True, 1.0, -1
    scale = float(destination) / float(source)
    for _ in range(destination):
        terms = []
        while scale < span:
            if next_row and number_rows < source:
                row += 1                                  # read a new scanline into x_vector
                number_rows += 1
            terms.append((row, scale))                    # y_vector += scale.y * x_vector
            span -= scale
            scale = float(destination) / float(source)
            next_row = True
        if next_row and number_rows < source:
            row += 1
            number_rows += 1
            next_row = False
        terms.append((row, span))                         # pixel = y_vector + span.y * x_vector
        scale -= span
        if scale <= 0:
            scale = float(destination) / float(source)
            next_row = True
        span = 1.0
        plan.append(terms)
    return plan


def plan_columns(source, destination):
    """resize.c:4419-4471.  Per destination column the terms whose running sum is the value last stored
    to scale_scanline[t].  None on the equal-columns path.  Raises when a store lands beyond the
    scanline or a column is never stored (the reference then misbehaves; no such geometry is known)."""
    if source == destination:
        return None
    stored = {}
    pixel = []
    next_column, span, t = False, 1.0, 0
    for x in range(source):
        scale = float(destination) / float(source)
        while scale >= span:
            if next_column:
                pixel = []
                t += 1
            pixel.append((x, span))
            if t >= destination:
                raise ValueError("store beyond the scanline")
            stored[t] = list(pixel)
            scale -= span
            span = 1.0
            next_column = True
        if scale > 0:
            if next_column:
                pixel = []
                next_column = False
                t += 1
            pixel.append((x, scale))
            span -= scale
    if span > 0:
        pixel.append((source - 1, span))
    if not next_column and t < destination:
        stored[t] = list(pixel)
    if sorted(stored) != list(range(destination)):
        raise ValueError("a destination column is never stored")
    return [stored[d] for d in range(destination)]


def sample_offsets(source, destination, percent=None):
    """resize.c:3952, :3969, :3984-3986."""
    offset = 0.5 - EPSILON if percent is None or percent < 0 else percent / 100.0 - EPSILON
    return np.array([int(((float(j) + offset) * source) / destination) for j in range(destination)], dtype=np.int64)


# -------------------------------------------------------------------------------------- restatement
def _clamp(values, dtype):
    """ClampToQuantum, quantum.h:86-97."""
    if dtype == np.float32:
        return values.astype(np.float32)
    with np.errstate(invalid="ignore"):
        out = np.floor(np.clip(values, 0.0, QR) + 0.5)
        out[~(values > 0.0)] = 0.0
        out[values >= QR] = QR
    return out.astype(np.uint16)


def _perceptible_reciprocal(x):
    sign = np.where(x < 0.0, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sign * x >= EPSILON, 1.0 / x, sign / EPSILON)


def _sums(values, plan, axis):
    """values along `axis` through the plan: every sum starts from 0.0, one multiply and one add a term."""
    if plan is None:
        return values
    shape = list(values.shape)
    shape[axis] = len(plan)
    out = np.empty(shape, dtype=np.float64)
    for d, terms in enumerate(plan):
        total = np.zeros_like(values[0] if axis == 0 else values[:, 0])
        for source, weight in terms:
            total = total + weight * (values[source] if axis == 0 else values[:, source])
        if axis == 0:
            out[d] = total
        else:
            out[:, d] = total
    return out


def restate_scale(px, rows, columns, has_alpha, blend=None):
    """ScaleImage.  blend: the stored offsets that carry the Blend trait (default: every channel but the
    alpha of a frame with alpha; a channel masked out by the channel mask carries Copy without Blend)."""
    channels = px.shape[2]
    if blend is None:
        blend = tuple(range(channels - 1)) if has_alpha else ()
    x = px.astype(np.float64)
    if has_alpha:
        alpha = QS * x[..., channels - 1]
        for c in blend:
            x[..., c] = alpha * x[..., c]
    scanlines = _sums(x, plan_rows(px.shape[0], rows), 0)
    scaled = _sums(scanlines, plan_columns(px.shape[1], columns), 1)
    if has_alpha:
        gamma = _perceptible_reciprocal(QS * scaled[..., channels - 1])
        scaled = scaled.copy()
        for c in blend:
            scaled[..., c] = gamma * scaled[..., c]
    return _clamp(scaled, px.dtype.type)


def restate_sample(px, rows, columns, offset=None):
    ox, oy = offset_percent(offset)
    return np.ascontiguousarray(px[sample_offsets(px.shape[0], rows, oy)][:, sample_offsets(px.shape[1], columns, ox)])
