"""TEST INFRASTRUCTURE — a plain fp64 NumPy restatement of the number MorphologyPrimitive returns: how many
samples one pass changed (MagickCore/morphology.c:2566-3227), for frames WITHOUT alpha weighting.

For every sample of every channel that carries the update trait the reference forms `pixel`, the UNROUNDED result:
  Convolve      bias + sum k*p over the non-NaN cells of the reflected kernel          (:2740-2754, :2899, :2938-2956)
  Erode         the minimum of the sample itself and the samples under cells >= 0.5      (:2910, :2990-3005)
  Dilate        the maximum of 0 and the samples under cells > 0.5, kernel reflected     (:2905, :3020-3035)
with the source clamped to its edge, counts it where |pixel - sample| >= MagickEpsilon (:2772, :3199) — before the
value is clamped and rounded to a Quantum — and returns the count divided by the number of channels that carry the
update trait (GetImageChannels, image-private.h:147-164; :2806, :3226).

The sums are formed in the order NumPy likes, not the reference's: the restatement is for inputs whose partial sums
are exact in fp64 whatever the order (integer cells, integer samples, biases that are multiples of 1/4)."""
import numpy as np

MAGICK_EPSILON = 1.0e-12
REFLECTED = {"convolve": True, "dilate": True, "erode": False}


def shifted(pixels, dy, dx):
    """out[y, x] = pixels[clamp(y + dy), clamp(x + dx)]: the edge virtual pixels of the reference's cache view."""
    rows, cols = pixels.shape[:2]
    ys = np.clip(np.arange(rows) + dy, 0, rows - 1)
    xs = np.clip(np.arange(cols) + dx, 0, cols - 1)
    return pixels[ys][:, xs]


def unrounded(pixels, method, values, x, y, bias=0.0):
    """`pixel` of every sample as it stands where the reference takes its count: float64 [rows, cols, channels]."""
    method = method.lower()
    reflected = REFLECTED[method]
    values = np.asarray(values, dtype=np.float64)
    h, w = values.shape
    px = np.asarray(pixels, dtype=np.float64)
    if px.ndim == 2:
        px = px[:, :, None]
    # where the window starts relative to the output pixel (offset.x / offset.y, :2611-2639)
    ox, oy = (w - x - 1, h - y - 1) if reflected else (x, y)
    if method == "convolve":
        out = np.full(px.shape, float(bias))
    elif method == "dilate":
        out = np.zeros(px.shape)
    else:
        out = px.copy()
    for v in range(h):
        for u in range(w):
            k = values[h - 1 - v, w - 1 - u] if reflected else values[v, u]
            if np.isnan(k):
                continue
            sample = shifted(px, v - oy, u - ox)
            if method == "convolve":
                out += k * sample
            elif method == "dilate":
                if k > 0.5:
                    out = np.maximum(out, sample)
            elif k >= 0.5:
                out = np.minimum(out, sample)
    return out


def changed_count(pixels, method, values, x, y, bias=0.0, copy_channels=()):
    """(samples, returned): the samples one pass counts as changed, and what MorphologyPrimitive returns for them."""
    px = np.asarray(pixels, dtype=np.float64)
    if px.ndim == 2:
        px = px[:, :, None]
    updated = [c for c in range(px.shape[2]) if c not in tuple(copy_channels)]
    differs = np.abs(unrounded(px, method, values, x, y, bias) - px) >= MAGICK_EPSILON
    samples = int(differs[:, :, updated].sum())
    return samples, samples // max(1, len(updated))
