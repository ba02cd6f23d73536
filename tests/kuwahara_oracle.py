"""KuwaharaImage on the compiled reference (the MagickCore entry point is called directly, as
edge_blur_oracle.py calls BilateralBlurImage), the inputs its tests share, and a NumPy restatement
of the selection behind the blur (effect.c:1836-1955, pixel.c:4975-5033) that also tells which
quadrant every pixel chose."""
import ctypes

import numpy as np

QS = 1.0 / 65535.0               # QuantumScale, magick-type.h:119
EPSILON = 1.0e-12                # MagickEpsilon

SHAPES = [(1, 1), (1, 40), (40, 1), (3, 3), (15, 17), (16, 16), (17, 33), (61, 97), (130, 70)]   # rows x columns
RADII = [0, 0.5, 1, 2, 3, 4, 7, 15]
SIGMAS = [0.5, 1.5, 3]
LAYOUTS = ["gray", "gray+alpha", "rgb", "rgba", "plain4"]
CHANNELS = {"gray": 1, "gray+alpha": 2, "rgb": 3, "rgba": 4, "plain4": 4}
SEED = 1775


def cases(shape_index):
    """The reduced cross product of one shape: every radius, the layout and the sigma stepping so
    that every value of every axis meets both Quantum types (the tests run each case on both)."""
    return [(radius, SIGMAS[(shape_index + 2 * i) % len(SIGMAS)], LAYOUTS[(shape_index + i) % len(LAYOUTS)])
            for i, radius in enumerate(RADII)]


def _bind(L):
    if getattr(L, "_kuwahara_bound", False):
        return L
    vp, dbl, cp = ctypes.c_void_p, ctypes.c_double, ctypes.c_char_p
    L.AcquireExceptionInfo.restype = vp
    L.AcquireExceptionInfo.argtypes = []
    L.DestroyExceptionInfo.restype = vp
    L.DestroyExceptionInfo.argtypes = [vp]
    L.KuwaharaImage.restype = vp
    L.KuwaharaImage.argtypes = [vp, dbl, dbl, vp]
    L.AcquireImageInfo.restype = vp
    L.AcquireImageInfo.argtypes = []
    L.DestroyImageInfo.restype = vp
    L.DestroyImageInfo.argtypes = [vp]
    L.SetImageOption.restype = ctypes.c_int
    L.SetImageOption.argtypes = [vp, cp, cp]
    L.SyncImageSettings.restype = ctypes.c_int
    L.SyncImageSettings.argtypes = [vp, vp, vp]
    L._kuwahara_bound = True
    return L


def ref_kuwahara(refmod, image, radius, sigma):
    """KuwaharaImage(image, radius, sigma) on a refmod.RefImage; returns a new RefImage."""
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    handle = L.KuwaharaImage(image.handle, float(radius), float(sigma), exception)
    L.DestroyExceptionInfo(exception)
    if not handle:
        raise RuntimeError("KuwaharaImage failed")
    return refmod.RefImage(handle=handle, lib=L, hdri=image.hdri)


def set_interpolate(image, method):
    """image->interpolate, as `-interpolate method` sets it (SyncImageSettings, image.c)."""
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    info = L.AcquireImageInfo()
    ok = L.SetImageOption(info, b"interpolate", method.encode()) and L.SyncImageSettings(info, image.handle, exception)
    L.DestroyImageInfo(info)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("interpolate method %r rejected" % method)
    return image


# ------------------------------------------------------------------------------------------ inputs
def noise(rows, cols, channels, dtype, seed=SEED):
    """Independent, identically distributed samples over the whole Quantum range."""
    rng = np.random.default_rng(seed + 1000 * rows + cols + 7 * channels)
    a = rng.integers(0, 65536, (rows, cols, channels), dtype=np.uint16)
    if dtype == np.float32:
        f = a.astype(np.float32) + rng.random((rows, cols, channels), dtype=np.float32)
        return np.ascontiguousarray(np.minimum(f, np.float32(65535.0)))
    return np.ascontiguousarray(a)


def sprite_alpha(px, fraction=0.6, seed=5):
    """The last channel becomes a sprite's alpha: `fraction` of its samples exactly 0."""
    rng = np.random.default_rng(seed)
    out = px.copy()
    out[..., -1][rng.random(px.shape[:2]) < fraction] = 0
    return out


def constant(rows, cols, channels, dtype, value=31000):
    return np.full((rows, cols, channels), value, dtype=dtype)


def flat_blocks(rows, cols, channels, dtype, block=32, seed=9):
    """Flat block x block squares of random levels."""
    rng = np.random.default_rng(seed)
    levels = rng.integers(0, 65536, ((rows + block - 1) // block, (cols + block - 1) // block, channels))
    return np.ascontiguousarray(np.kron(levels, np.ones((block, block, 1), dtype=np.int64))[:rows, :cols].astype(dtype))


def step_edge(rows, cols, channels, dtype, low=9000, high=52000):
    """A vertical step edge, no noise."""
    a = np.full((rows, cols, channels), low, dtype=dtype)
    a[:, cols // 2:] = high
    return a


def wide_range_float(rows, cols, channels, seed=3):
    """Float samples spanning 1e-3 ... 6e4 in one frame: the order of a sum shows in its last bits."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((10.0 ** rng.uniform(-3.0, np.log10(6.0e4), (rows, cols, channels))).astype(np.float32))


def out_of_range_float(rows, cols, channels, seed=4):
    """Float samples below 0 and above QuantumRange."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-20000.0, 90000.0, (rows, cols, channels)).astype(np.float32))


# -------------------------------------------------------------------------------------- restatement
def _perceptible_reciprocal(x):
    sign = np.where(x < 0.0, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sign * x >= EPSILON, 1.0 / x, sign / EPSILON)


def _clamp(values, dtype):
    if dtype == np.float32:
        return values.astype(np.float32)
    out = np.floor(np.clip(values, 0.0, 65535.0) + 0.5)
    out[~(values > 0.0)] = 0.0
    out[values >= 65535.0] = 65535.0
    return out.astype(np.uint16)


def restate(blurred, radius, blend=None, alpha=None, gray=None):
    """The part of KuwaharaImage behind gaussian_image=BlurImage(...), on that blurred frame.

    blend: the channels whose trait carries Blend (default: every channel but the last when the
    layout has 2 or 4 channels); alpha: the channel GetPixelAlpha reads (default: the last of a 2-
    or 4-channel layout, else None = OpaqueAlpha); gray: R, G and B at offset 0 (default: fewer
    than three channels).  Returns (kuwahara frame, chosen quadrant per pixel)."""
    rows, cols, channels = blurred.shape
    if alpha is None and blend is None and channels in (2, 4):
        alpha = channels - 1
    if blend is None:
        blend = [c for c in range(channels) if alpha is not None and c != alpha]
    if gray is None:
        gray = channels < 3
    w = int(radius) + 1
    reach, after = w - 1, max(w - 1, w // 2 + 1)         # the 2 x 2 fetch reaches a pixel past the windows for w <= 2
    P = np.pad(blurred.astype(np.float64), ((reach, after), (reach, after), (0, 0)), mode="edge")
    r, g, b = (0, 0, 0) if gray else (0, 1, 2)
    luma = 0.212656 * P[..., r] + 0.715158 * P[..., g] + 0.072186 * P[..., b]
    mh, mw = rows + reach, cols + reach                      # distinct windows, by origin
    mean = np.zeros((mh, mw, channels))
    for v in range(w):
        for u in range(w):
            mean += P[v:v + mh, u:u + mw]
    mean /= float(w * w)
    mean_luma = 0.212656 * mean[..., r] + 0.715158 * mean[..., g] + 0.072186 * mean[..., b]
    variance = np.zeros((mh, mw))
    for v in range(w):
        for u in range(w):
            d = luma[v:v + mh, u:u + mw] - mean_luma
            variance += d * d
    yy, xx = np.mgrid[0:rows, 0:cols]
    best = variance[yy, xx].copy()
    quadrant = np.zeros((rows, cols), dtype=np.int64)
    oy, ox = yy.copy(), xx.copy()
    for q, (dy, dx) in enumerate([(0, reach), (reach, 0), (reach, reach)], start=1):
        candidate = variance[yy + dy, xx + dx]
        wins = candidate < best
        best = np.where(wins, candidate, best)
        quadrant[wins] = q
        oy[wins] = (yy + dy)[wins]
        ox[wins] = (xx + dx)[wins]
    half = w // 2
    delta = 0.5 * (w & 1)
    epsilon = 1.0 - delta
    py, px = oy + half, ox + half
    p = [P[py, px], P[py, px + 1], P[py + 1, px], P[py + 1, px + 1]]
    if alpha is None:
        a = [np.full((rows, cols), QS * 65535.0)] * 4
    else:
        a = [QS * t[..., alpha] for t in p]
    out = np.empty((rows, cols, channels))
    for c in range(channels):
        t = [s[..., c] for s in p]
        if c in blend:
            t = [t[i] * a[i] for i in range(4)]
            gamma = epsilon * (epsilon * a[0] + delta * a[1]) + delta * (epsilon * a[2] + delta * a[3])
        else:
            gamma = np.full((rows, cols), epsilon * (epsilon + delta) + delta * (epsilon + delta))
        gamma = _perceptible_reciprocal(gamma)
        out[..., c] = gamma * (epsilon * (epsilon * t[0] + delta * t[1]) + delta * (epsilon * t[2] + delta * t[3]))
    return _clamp(out, blurred.dtype.type), quadrant


def plain4_reference(refmod, px, radius, sigma):
    """Four channels without an alpha trait (CMYK's layout): the reference blurs every channel on its
    own, so the blurred frame is its RGB blur of the first three channels beside its gray blur of
    the fourth; the selection reads R, G and B and interpolates all four plainly."""
    blurred = np.concatenate([refmod.RefImage(px[:, :, :3].copy()).blur(radius, sigma).numpy(),
                              refmod.RefImage(px[:, :, 3].copy()).blur(radius, sigma).numpy().reshape(px.shape[:2] + (1,))],
                             axis=2)
    want, _ = restate(blurred, radius, blend=[], alpha=None, gray=False)
    rgb = ref_kuwahara(refmod, refmod.RefImage(px[:, :, :3].copy()), radius, sigma).numpy()
    assert np.array_equal(np.ascontiguousarray(want[..., :3]).view(np.uint8), rgb.view(np.uint8)), "the restatement left the reference"
    return want
