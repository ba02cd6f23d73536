"""CLAHEImage on the compiled reference (the MagickCore entry point is called directly, as
kuwahara_oracle.py calls KuwaharaImage), the inputs and the case list its tests share, and a NumPy
restatement of what the operator does between its two colourspace transforms (enhance.c:295-614,
:660-780) on an L plane."""
import ctypes

import numpy as np

# rows, columns, tile width, tile height
SHAPES = [(16, 16, 0, 0),          # 2 x 2 tiles: the limit clamps to 1
          (64, 64, 8, 8),          # no padding
          (61, 97, 16, 16),        # odd padding: 7 columns left, 8 right
          (33, 50, 7, 5),          # odd tiles: the w>>1 / (w+1)>>1 border regions differ
          (20, 30, 64, 64),        # a tile larger than the frame: a 1 x 1 grid
          (40, 40, 1, 1),          # the left and top border regions are empty
          (40, 40, 2, 3),
          (1030, 2051, 0, 0)]      # 256 x 128 tiles: several workgroups bin one tile
BINS = [0, 2, 3, 128, 255, 256, 300]
CLIPS = [0.5, 1.0, 1.5, 2.0, 4.0, 1e6]
SEED = 616

# (number_bins, clip_limit, channels) per shape: a reduced cross product in which every value of
# every axis occurs, and every case runs on both Quantum types.  The library declines a frame whose
# tile maps (tiles x bins x 2 bytes) are larger than the frame itself, so the shapes with many
# small tiles meet the small bin counts (the Q16 frame is the smaller one: it decides).
_CASES = [[(2, 0.5, 4), (3, 2.0, 3)],
          [(128, 2.0, 3), (256, 1.5, 4), (255, 4.0, 4), (0, 1.0, 3)],
          [(0, 2.0, 4), (300, 0.5, 3), (255, 1.5, 3), (3, 1e6, 4), (2, 4.0, 3), (128, 1.0, 4)],
          [(2, 2.0, 3), (3, 0.5, 4)],
          [(256, 2.0, 3), (300, 4.0, 4), (0, 0.5, 3), (128, 1e6, 4)],
          [(2, 2.0, 4), (3, 0.5, 4)],
          [(3, 1.5, 3), (2, 4.0, 4)],
          [(0, 2.0, 4), (256, 4.0, 3)]]


def cases(shape_index):
    return list(_CASES[shape_index])


def resolved_bins(number_bins):
    return 128 if number_bins == 0 else min(number_bins, 256)


def geometry(rows, cols, width, height):
    """(tile width, tile height, pad_x, pad_y): enhance.c:662-673."""
    tw = width if width else cols >> 3
    th = height if height else rows >> 3
    pad_x = tw - cols % tw if cols % tw else 0
    pad_y = th - rows % th if rows % th else 0
    return tw, th, pad_x, pad_y


def table_fits(rows, cols, channels, dtype, width, height, number_bins):
    """The library's condition: tiles x bins x 2 bytes no larger than the frame."""
    tw, th, pad_x, pad_y = geometry(rows, cols, width, height)
    tiles = ((cols + pad_x) // tw) * ((rows + pad_y) // th)
    return tiles * resolved_bins(number_bins) * 2 <= rows * cols * channels * np.dtype(dtype).itemsize


def _bind(L):
    if getattr(L, "_clahe_bound", False):
        return L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.AcquireExceptionInfo.restype = vp
    L.AcquireExceptionInfo.argtypes = []
    L.DestroyExceptionInfo.restype = vp
    L.DestroyExceptionInfo.argtypes = [vp]
    L.CLAHEImage.restype = ctypes.c_int
    L.CLAHEImage.argtypes = [vp, sz, sz, sz, ctypes.c_double, vp]
    L._clahe_bound = True
    return L


def ref_clahe(image, width, height, number_bins, clip_limit):
    """CLAHEImage(image, width, height, number_bins, clip_limit) on a refmod.RefImage, in place."""
    L = _bind(image.L)
    exception = L.AcquireExceptionInfo()
    ok = L.CLAHEImage(image.handle, int(width), int(height), int(number_bins), float(clip_limit), exception)
    L.DestroyExceptionInfo(exception)
    if not ok:
        raise RuntimeError("CLAHEImage failed")
    return image


_REFERENCES = {}


def reference(refmod, px, colorspace, width, height, number_bins, clip_limit, key=None):
    """The compiled reference's CLAHEImage of px; with a key, computed once and shared (read-only)."""
    if key is not None:
        key = (key, px.shape, px.dtype.name, colorspace, width, height, number_bins, clip_limit)
        if key in _REFERENCES:
            return _REFERENCES[key]
    want = ref_clahe(refmod.RefImage(px, colorspace=colorspace), width, height, number_bins, clip_limit).numpy()
    want.setflags(write=False)
    if key is not None:
        _REFERENCES[key] = want
    return want


# ------------------------------------------------------------------------------------------ inputs
def noise(rows, cols, channels, dtype, seed=SEED):
    """Independent, identically distributed samples over the whole Quantum range."""
    rng = np.random.default_rng(seed + 1000 * rows + cols + 7 * channels)
    a = rng.integers(0, 65536, (rows, cols, channels), dtype=np.uint16)
    if dtype == np.float32:
        f = a.astype(np.float32) + rng.random((rows, cols, channels), dtype=np.float32)
        return np.ascontiguousarray(np.minimum(f, np.float32(65535.0)))
    return np.ascontiguousarray(a)


def constant(rows, cols, channels, dtype, value=31000):
    """Everything in one bin: the most clipping and redistribution."""
    return np.full((rows, cols, channels), value, dtype=dtype)


def flat_blocks(rows, cols, channels, dtype, block=32, seed=9):
    """Flat block x block squares of random levels."""
    rng = np.random.default_rng(seed)
    levels = rng.integers(0, 65536, ((rows + block - 1) // block, (cols + block - 1) // block, channels))
    return np.ascontiguousarray(np.kron(levels, np.ones((block, block, 1), dtype=np.int64))[:rows, :cols].astype(dtype))


def gradient(rows, cols, channels, dtype):
    """A horizontal ramp over the whole range: neighbouring lanes share bins."""
    ramp = np.round(np.linspace(0.0, 65535.0, cols))
    return np.ascontiguousarray(np.broadcast_to(ramp[None, :, None], (rows, cols, channels)).astype(dtype))


def band(rows, cols, channels, dtype, number_bins=128, seed=12):
    """Noise confined to three neighbouring bins of a number_bins histogram."""
    delta = 65535 // resolved_bins(number_bins) + 1
    rng = np.random.default_rng(seed)
    low = 40 * delta if 43 * delta <= 65536 else 0
    return np.ascontiguousarray(rng.integers(low, min(low + 3 * delta, 65536), (rows, cols, channels)).astype(dtype))


def float_specials(rows, cols, channels, seed=4):
    """Float Quantum only: negatives, values above QuantumRange and exact x.5 values."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-20000.0, 90000.0, (rows, cols, channels)).astype(np.float32)
    halves = rng.random((rows, cols, channels)) < 0.4
    a[halves] = (rng.integers(0, 65535, int(halves.sum())) + 0.5).astype(np.float32)
    a[0, 0, 0], a[0, 1, 0], a[0, 2, 0] = -0.0, 65534.5, 65535.0
    return np.ascontiguousarray(a)


INPUTS = {"noise": noise, "constant": constant, "flat blocks": flat_blocks, "gradient": gradient, "band": band}


# -------------------------------------------------------------------------------------- restatement
def scale_quantum_to_short(plane):
    """quantum-private.h:517-528."""
    if plane.dtype == np.uint16:
        return plane.astype(np.int64)
    with np.errstate(invalid="ignore"):
        rounded = (plane + np.float32(0.5)).astype(np.float32)
        inside = (plane > 0) & (plane < np.float32(65535.0))
        out = np.where(inside, rounded, 0).astype(np.int64)
    out[plane >= np.float32(65535.0)] = 65535
    return out


def clip_histogram(limit, histogram):
    """ClipCLAHEHistogram (enhance.c:302-375), statement for statement, on a list of ints;
    limit is the (integral) double the reference passes."""
    bins = len(histogram)
    cumulative_excess = 0
    for i in range(bins):
        excess = histogram[i] - limit
        if excess > 0:
            cumulative_excess += excess
    step = cumulative_excess // bins
    excess = limit - step
    for i in range(bins):
        if histogram[i] > limit:
            histogram[i] = limit
        elif histogram[i] > excess:
            cumulative_excess -= histogram[i] - excess
            histogram[i] = limit
        else:
            cumulative_excess -= step
            histogram[i] += step
    while True:
        previous_excess = cumulative_excess
        p = 0
        while cumulative_excess != 0 and p < bins:
            step = int(bins / cumulative_excess) if cumulative_excess < 0 else bins // cumulative_excess   # C division
            if step < 1:
                step = 1
            p = 0
            while p < bins and cumulative_excess != 0:
                if histogram[p] < limit:
                    histogram[p] += 1
                    cumulative_excess -= 1
                p += step
            p += 1
        if not (cumulative_excess != 0 and cumulative_excess < previous_excess):
            break
    return histogram


def map_histogram(histogram, number_pixels):
    """MapCLAHEHistogram (enhance.c:453-475) with range 0 ... 65535."""
    scale = 65535.0 / number_pixels
    total = 0.0
    out = []
    for count in histogram:
        total += float(count)
        out.append(min(int(0 + scale * total), 65535))
    return np.array(out, dtype=np.int64)


def _regions(tiles, tile):
    """(origin, extent, near tile, far tile) of the tiles+1 regions along one axis (enhance.c:544-600)."""
    out = [(0, tile >> 1, 0, 0)]
    for i in range(1, tiles):
        out.append(((tile >> 1) + (i - 1) * tile, tile, i - 1, i))
    out.append(((tile >> 1) + (tiles - 1) * tile, (tile + 1) >> 1, tiles - 1, tiles - 1))
    return out


def restate(plane, width, height, number_bins, clip_limit):
    """CLAHEImage's steps between the colourspace transforms on channel 0 (rows x columns, uint16 or
    float32): returns the plane the reference writes back."""
    rows, cols = plane.shape
    tw, th, pad_x, pad_y = geometry(rows, cols, width, height)
    left, top = pad_x >> 1, pad_y >> 1
    P = np.pad(scale_quantum_to_short(plane), ((top, pad_y - top), (left, pad_x - left)), mode="edge")
    if clip_limit != 1.0:
        bins = resolved_bins(number_bins)
        tiles_x, tiles_y = P.shape[1] // tw, P.shape[0] // th
        delta = (65535 // bins + 1) & 0xFFFF
        lut = P // delta
        limit = int(clip_limit * float(tw * th) / float(bins))
        limit = max(limit, 1)
        maps = np.empty((tiles_y, tiles_x, bins), dtype=np.int64)
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                counts = np.bincount(lut[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=bins)
                maps[ty, tx] = map_histogram(clip_histogram(limit, [int(c) for c in counts]), tw * th)
        out = P.copy()
        for y0, H, near_y, far_y in _regions(tiles_y, th):
            for x0, W, near_x, far_x in _regions(tiles_x, tw):
                if W == 0 or H == 0:
                    continue
                b = lut[y0:y0 + H, x0:x0 + W]
                q12, q22 = maps[near_y, near_x][b].astype(np.float64), maps[near_y, far_x][b].astype(np.float64)
                q11, q21 = maps[far_y, near_x][b].astype(np.float64), maps[far_y, far_x][b].astype(np.float64)
                x = (W - np.arange(W, dtype=np.float64))[None, :]
                y = (H - np.arange(H, dtype=np.float64))[:, None]
                value = (1.0 / (float(W) * float(H))) * (y * (x * q12 + (float(W) - x) * q22) +
                                                         (float(H) - y) * (x * q11 + (float(W) - x) * q21))
                out[y0:y0 + H, x0:x0 + W] = value.astype(np.int64) & 0xFFFF
        P = out
    return P[top:top + rows, left:left + cols].astype(plane.dtype)


def restate_frame(px, width, height, number_bins, clip_limit):
    """... on an interleaved Lab frame: channel 0 replaced, the others untouched."""
    out = px.copy()
    out[..., 0] = restate(px[..., 0], width, height, number_bins, clip_limit)
    return out
