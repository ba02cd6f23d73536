#!/usr/bin/env python3
"""Randomised differential run against the compiled reference.  tests/test_gpu_stress_slice.py runs a fixed-seed
slice of every operator family below inside the suite; this script runs them for as long as asked.  Shapes, kernel lengths and operators are drawn at random, every result
is compared with the reference: FAST blur / unsharp within +-1 (unsharp: 1+gain off the threshold
edge), EXACT and the morphology / histogram operators bit-identical.
   python tests/stress_parity.py [seconds] [seed]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tests/ -> repository root
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import imagemagick_amd as im
from oracle import ref as refmod
import statistic_oracle
import edge_blur_oracle
import kuwahara_oracle
import clahe_oracle
import threshold_oracle
import levels_oracle
import scale_oracle
from test_gpu_adaptive_threshold import BIASES as ADAPTIVE_BIASES
from test_gpu_levels import LIBM_SHARE, level_libm

rng = np.random.default_rng(1)
_ready = False


def setup(seed=1):
    """Load the library (once), pin the starting precision, reseed the case generator and restart the case counters."""
    global rng, _ready
    rng = np.random.default_rng(seed)
    declined.clear()
    drawn.clear()
    if not _ready:
        im.load()
        refmod.set_thread_limit(os.cpu_count() or 1)
        im.set_option("MAGICKHIP_RESIZE_ONE_LAUNCH_MIN_PIXELS", "0")     # small frames through the one-launch resize kernels too
        im.set_option("MAGICKHIP_GRAY_BANDS_MIN_PIXELS", "0")            # ... and small gray frames through the four-band form of the fused blur
        im.set_option("MAGICKHIP_RGB_PAD_MIN_PIXELS", "0")               # ... small RGB frames through the padded form of Erode / Dilate
        im.set_option("MAGICKHIP_RGB_PAD_FLOAT_ALWAYS", "1")             #     (float: also under kernels morph_convex would take)
        _ready = True
    im.set_precision(im.PRECISION_EXACT)           # (the library's default is FAST; the cases below switch per call)


def dev(px, **kw):
    t = torch.from_numpy(px.view(np.int16)).cuda().view(torch.uint16)
    return im.Image(t, **kw)


def pixels(rows, cols, kind):
    px = rng.integers(0, 65536, (rows, cols, 4), dtype=np.uint16)
    if kind == 1:
        px[:, :, 3] = 65535
    elif kind == 2:
        px[:, :, 3] = rng.integers(0, 4, (rows, cols), dtype=np.uint16)          # tiny alpha
    elif kind == 3:
        px[:, :, 3] = np.where(rng.random((rows, cols)) < 0.5, 0, 65535)          # binary alpha
    elif kind == 4:
        px[:] = (np.add.outer(np.arange(rows), np.arange(cols)) % 2 * 40000 + 100)[:, :, None]
    elif kind == 5:                                # a sprite: opaque rectangles on a transparent ground
        px[:, :, 3] = 0
        for _ in range(6):
            y, x = int(rng.integers(0, max(1, rows - 2))), int(rng.integers(0, max(1, cols - 2)))
            px[y: y + int(rng.integers(1, 25)), x: x + int(rng.integers(1, 25)), 3] = 65535
    return px


def dev_float(px, **kw):
    return im.Image(torch.from_numpy(px).cuda(), **kw)


def float_pixels(rows, cols, kind):
    """Float Quantum frames: fractional levels, values beyond the Quantum range and below zero,
    small / zero alpha, neighbouring floats (values on float-rounding midpoints after a blur)."""
    px = (rng.random((rows, cols, 4)) * 65535.0).astype(np.float32)
    if kind == 1:
        px[:, :, 3] = 65535.0
    elif kind == 2:
        px[:, :, 3] = (10.0 ** rng.uniform(-9, 0, (rows, cols))).astype(np.float32)
    elif kind == 3:
        px[:, :, :3] = (rng.random((rows, cols, 3)) * 90000.0 - 12000.0).astype(np.float32)
        px[:, :, 3] = np.where(rng.random((rows, cols)) < 0.3, 0.0, 65535.0)
    elif kind == 5:                                # a sprite: opaque rectangles on a transparent ground
        px[:, :, 3] = 0.0
        for _ in range(6):
            y, x = int(rng.integers(0, max(1, rows - 2))), int(rng.integers(0, max(1, cols - 2)))
            px[y: y + int(rng.integers(1, 25)), x: x + int(rng.integers(1, 25)), 3] = 65535.0
    elif kind == 4:
        low = np.float32(rng.uniform(1.0, 60000.0))
        board = (np.add.outer(np.arange(rows), np.arange(cols)) % 2) == 1
        px[:, :, :3] = np.where(board, np.nextafter(low, np.float32(np.inf)), low)[:, :, None]
        px[:, :, 3] = 65535.0
    return px


def check_bits(name, got, want, detail):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same)
        print("MISMATCH %s %s: %d float samples differ, first at %s: %r vs %r" % (
            name, detail, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]), flush=True)
        return 1
    return 0


def check_ulp(name, got, want, limit, detail, residue=0.0):
    """Float results within `limit` float ULPs of the reference's (same NaN pattern, same infinities), or —
    the residue of a cancellation, 1e-20 out of terms of 1e-8 — within `residue` absolutely."""
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        print("MISMATCH %s %s: NaN pattern differs" % (name, detail), flush=True)
        return 1
    if residue > 0.0:
        with np.errstate(invalid="ignore"):
            close = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= residue
        got = np.where(close, want, got)
    def ordered(a):
        bits = np.nan_to_num(a, nan=0.0).view(np.int32).astype(np.int64)
        return np.where(bits < 0, -(bits & 0x7fffffff), bits)
    d = np.abs(ordered(got) - ordered(want))
    if d.max(initial=0) > limit:
        bad = np.argwhere(d > limit)
        print("MISMATCH %s %s: max %d ULP (limit %d), %d samples, first at %s: %r vs %r" % (
            name, detail, d.max(), limit, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]), flush=True)
        return 1
    return 0


def check(name, got, want, limit, detail):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if d.max(initial=0) > limit:
        bad = np.argwhere(d > limit)
        print("MISMATCH %s %s: max %d (limit %d), %d samples, first at %s" % (
            name, detail, d.max(), limit, len(bad), bad[0].tolist()), flush=True)
        return 1
    return 0


# STRESS_OPS=0,1,2 restricts the operators (0 FAST blur, 1 EXACT blur, 2 FAST unsharp, 3 Erode/Dilate on RGBA, gray
# (four row bands) and RGB (a fourth, empty channel) frames, 4 histogram operators, 5 FAST 2-D convolve on the same three
# layouts, 6 FAST Lab, 7 EXACT GaussianBlur / Sharpen (separable +
# tie check), 8 float-Quantum blur / unsharp, 9 float-Quantum Erode / Dilate (RGBA and RGB), 10 float-Quantum
# GaussianBlur / Sharpen, 11 float-Quantum ContrastStretch / Equalize, 12 integer-cell 2-D convolve on the
# i8 matrix cores in both modes and three layouts, 13 2-D convolve with random real cells on every layout and
# Quantum type: the fused fp64 kernel, 14 ResizeImage: whole-number enlargements (one launch on the vector
# pipe under FAST), other enlargements (matrix pipe), reductions and mixed geometries, Q16 and float,
# alpha-weighted or four plain channels, both modes, 15 FAST BlurImage / GaussianBlurImage / UnsharpMaskImage on
# every layout: gray, gray + alpha, RGB, RGBA, four plain channels, 16 the pointwise enhance operators (FunctionImage,
# ContrastImage, ModulateImage, GrayscaleImage) with random parameters, colourspace and channel mask, 17 MotionBlurImage /
# RotationalBlurImage on every layout, alpha kind and shapes from 1 to 600 per side, 18 LocalContrastImage / DespeckleImage /
# WaveletDenoiseImage on shapes from 33 to 600 per side; 16 to 18 draw both Quantum types, 19 StatisticImage: every type, windows
# from 0 to the LDS limit with the three rank routes' boundaries at a fixed share, 20 BilateralBlurImage / SelectiveBlurImage,
# 21 KuwaharaImage, 22 CLAHEImage: the whole operator on Q16 sRGB frames and the core on Lab ones, 23 the six threshold operators,
# AdaptiveThresholdImage over more than one strip and band included, 24 the ten level operators, 25 SampleImage / ScaleImage /
# ThumbnailImage; 19 to 25 draw both Quantum types, both precision modes, host and device memory, every layout the operator's own
# tests run and a channel mask in half the cases, and nothing in them may be declined)
NUMBER_OF_OPS = 26

# families 16 to 18: cases the library declined / cases run, per family.  A declined case passes only when the decline
# condition stated in effects.hip holds for it, and at most a quarter of a family's cases may be declined.
declined = {}
drawn = {}


def blur_radius(sigma):
    """BlurImage's radius argument: 0 (the width from the sigma, gem.c:281-299) most of the time; otherwise a
    radius of its own — short ones cut the Gaussian off, long ones give kernels whose outer taps the reference
    zeroes (|t| < 1e-12, morphology.c:2494-2495) or leaves tiny."""
    if rng.random() < 0.6:
        return 0.0
    return float(np.ceil(rng.uniform(1.0, min(40.0, 6.0 * sigma + 4.0))))


def draw_frame():
    """The frame every case starts from (families 16 to 18 draw their own after it)."""
    rows, cols = int(rng.integers(1, 260)), int(rng.integers(1, 330))
    if rng.random() < 0.2:
        rows, cols = int(rng.integers(1, 40)), int(rng.integers(300, 1400))
    kind = int(rng.integers(0, 6))
    return rows, cols, kind, pixels(rows, cols, kind)


def enhance_frame(rows, cols, channels, is_float, kind):
    frame = float_pixels(rows, cols, kind) if is_float else pixels(rows, cols, kind)
    return np.ascontiguousarray(frame[:, :, 4 - channels:] if channels == 2 else frame[:, :, :channels])


def draw_enhance_case(op):
    """The inputs of one case of family 16, 17 or 18, drawn without touching the GPU (tests/test_enhance_edge_sizes.py
    draws a few hundred to check the share of declined cases); "declines": the library's stated condition holds."""
    case = {"op": op, "float": bool(rng.random() < 0.5), "kind": int(rng.integers(0, 6)), "declines": False,
            "mask": None, "copy": (), "colorspace": "sRGB", "libm": False}
    if op == 16:
        rows, cols = int(rng.integers(1, 260)), int(rng.integers(1, 330))
        channels = 4 if rng.random() < 0.6 else 3
        which = int(rng.integers(0, 4))
        if which == 0:
            function = ["Polynomial", "Sinusoid", "Arcsin", "Arctan"][int(rng.integers(0, 4))]
            count = int(rng.integers(1, 5))
            params = tuple(float(v) for v in rng.uniform(-1.5, 1.5, count)) if function == "Polynomial" else \
                tuple(float(v) for v in (rng.uniform(0.2, 5.0), rng.uniform(-180.0, 180.0) if function == "Sinusoid" else rng.uniform(0.0, 1.0),
                                         rng.uniform(0.1, 1.0), rng.uniform(0.0, 1.0))[:count])
            case.update(name="function", args=(function, params), libm=function != "Polynomial")
        elif which == 1:
            case.update(name="contrast", args=(bool(rng.random() < 0.5),), libm=True)
        elif which == 2:
            # percentages off the multiples of ten (those put results on exact rounding ties, test_modulate_colour_models)
            percent = tuple(float(v) for v in np.round(rng.uniform(3.0, 197.0, 3), 3))
            percent = tuple(v + 0.377 if v % 10.0 == 0.0 else v for v in percent)
            case.update(name="modulate", args=percent + (["HSL", "HSB"][int(rng.integers(0, 2))],))
        else:
            method = ["Rec709Luma", "Rec601Luma", "Rec709Luminance", "Rec601Luminance", "Average", "Brightness", "Lightness",
                      "MS", "RMS"][int(rng.integers(0, 9))]
            case.update(name="grayscale", args=(method,), colorspace=["sRGB", "RGB"][int(rng.integers(0, 2))])
        if rng.random() < 0.5:
            letters = "RGBA"[:channels]
            keep = [c for c in range(channels) if rng.random() < 0.5] or [int(rng.integers(0, channels))]
            case.update(mask="".join(letters[c] for c in keep), copy=tuple(c for c in range(channels) if c not in keep))
    elif op == 17:
        rows, cols = int(rng.integers(1, 601)), int(rng.integers(1, 601))
        channels = int(rng.integers(1, 5))
        if rng.random() < 0.5:
            sigma = float(rng.uniform(0.3, 8.0))
            radius = 0.0 if rng.random() < 0.6 else float(np.ceil(rng.uniform(1.0, 3.0 * sigma + 2.0)))
            case.update(name="motion_blur", args=(radius, sigma, float(rng.uniform(-360.0, 360.0))))
        else:
            # (small angles often: the sample count grows with the angle and the reference's CPU time with it)
            angle = float(rng.uniform(-360.0, 360.0)) if rng.random() < 0.3 else float(rng.uniform(-20.0, 20.0))
            # effect.c:3188-3199, :3262-3267: n = |4*radians*sqrt(blur_radius) + 2| samples per pixel.  A small negative angle gives
            # n = 0 (the reference fails to allocate its tables) or n = 1 (its pixel loop steps by n-1 = 0 and never
            # ends); the library declines both.  There is nothing to compare there: the mirrored angle instead
            blur_radius = float(np.hypot((cols - 1) / 2.0, (rows - 1) / 2.0))
            if int(abs(4.0 * np.pi * angle / 180.0 * np.sqrt(blur_radius) + 2.0)) < 2:
                angle = -angle
            case.update(name="rotational_blur", args=(angle,))
    else:
        rows, cols = int(rng.integers(33, 601)), int(rng.integers(33, 601))
        channels = int(rng.integers(1, 5))
        which = int(rng.integers(0, 3))
        if which == 0:
            # a blur width from below 1 (declined) to a little above half the columns (declined from (columns-2)/2 on)
            longest = max(rows, cols)
            radius = float(rng.uniform(0.7, 0.55 * cols)) / (0.002 * longest) * (1.0 if rng.random() < 0.8 else -1.0)
            w = int(longest * 0.002 * abs(radius))                   # launch_local_contrast, effects.hip
            case.update(name="local_contrast", args=(radius, float(rng.uniform(-100.0, 100.0))),
                        declines=(w < 1) or (cols <= 2 * w + 2))
        elif which == 1:
            case.update(name="despeckle", args=())
        else:
            case.update(name="wavelet_denoise", args=(float(rng.uniform(50.0, 12000.0)), float(rng.uniform(0.0, 1.0))),
                        declines=(rows < 33) or (cols < 33))              # launch_wavelet_denoise
    case["frame"] = enhance_frame(rows, cols, channels, case["float"], case["kind"])
    drawn[op] = drawn.get(op, 0) + 1
    if case["declines"]:
        declined[op] = declined.get(op, 0) + 1
    return case


def run_enhance_case(case):
    """Families 16 to 18 against the compiled reference: bit-identical; where the device's sin / asin / atan is involved
    Q16 within one level and float within one ULP."""
    frame, name, args, op = case["frame"], case["name"], case["args"], case["op"]
    what = "%s %s %dx%dx%d kind %d mask %s %s" % (args, frame.dtype.name, frame.shape[0], frame.shape[1], frame.shape[2],
                                                  case["kind"], case["mask"], case["colorspace"])
    reference = refmod.RefImage(frame, case["colorspace"])
    if case["mask"]:
        reference.set_channel_mask(case["mask"])
    image = (dev_float if case["float"] else dev)(frame, colorspace=case["colorspace"], copy_channels=case["copy"])
    try:
        got = getattr(im, name + "_image")(image, *args).numpy()
    except im.MagickHipError as error:
        if case["declines"] and 4 * declined[op] <= max(drawn[op], 12):
            return 0
        print("MISMATCH %s %s: declined (%s); stated condition holds: %s, %d of %d cases declined" % (
            name, what, error, case["declines"], declined.get(op, 0), drawn[op]), flush=True)
        return 1
    if case["declines"]:
        print("MISMATCH %s %s: the stated decline condition holds and the call went through" % (name, what), flush=True)
        return 1
    want = getattr(reference, name)(*args).numpy()
    if name == "grayscale":                     # the reference re-lays the frame out as gray[+alpha]; ours keeps G and B
        keep = [0] + ([frame.shape[2] - 1] if frame.shape[2] == 4 else [])
        got, want = np.ascontiguousarray(got[:, :, keep]), np.ascontiguousarray(want.reshape(frame.shape[0], frame.shape[1], -1)[:, :, [0, -1][:len(keep)]])
    got = got.reshape(want.shape)
    if case["float"]:
        return check_ulp(name, got, want, 1, what) if case["libm"] else check_bits(name, got, want, what)
    return check(name, got, want, 1 if case["libm"] else 0, what)


# ------------------------------------------------------------------------------------------------ families 19 to 25
# Every draw_*_case below builds its whole case on the host (tests/test_stress_draws.py draws a few hundred of each without a
# GPU); a case is inside the operator's stated domain, so run_domain_case counts a MagickHipError as a mismatch.
LAYOUT_CHANNELS = {"gray": 1, "gray+alpha": 2, "rgb": 3, "rgba": 4, "plain4": 4}
MASK_LETTERS = {1: "R", 2: "RA", 3: "RGB", 4: "RGBA"}                  # gray is the red channel (pixel.h:49-78)
MASK_BITS = {"R": 0x1, "G": 0x2, "B": 0x4, "A": 0x10}
# StatisticImage: the rank routes switch at W*H = 16 and 32 (launch_statistic); one case in three walks this table in
# order with a rank type, so 15 / 16 / 17 and 31 / 32 / 33 all come within a dozen cases
STATISTIC_ROUTE_WINDOWS = [(4, 4), (17, 1), (8, 4), (3, 11), (5, 3), (1, 31), (2, 8), (1, 17), (32, 1), (33, 1), (16, 1), (2, 16)]
STATISTIC_WORK = 1.5e6              # samples x window cells of one case: the reference's CPU time stays at tens of milliseconds
EDGE_BLUR_WORK = 6.0e6
SELECTIVE_INTENSITIES = [None, "Average", "Rec709Luminance", "Brightness"]      # test_selective_image_settings
KUWAHARA_RADII = [0, 0.5, 1, 1.5, 2, 3, 4, 5, 7]
CLAHE_BINS = [0, 2, 3, 64, 128, 255, 256, 300]
CLAHE_CLIPS = [0.5, 1.0, 1.5, 2.0, 4.0, 1e6]
THRESHOLD_OPERATORS = ["bilevel", "black", "white", "range", "auto", "adaptive"]
COLOUR_LAYOUTS = ["rgb", "rgba", "plain4"]                            # Black / White / Range decline a gray frame
ADAPTIVE_SPAN, ADAPTIVE_BAND_ROWS, ADAPTIVE_MAX_WIDTH = 512, 64, 257   # threshold.hip; test_stress_draws.py reads them there
LEVEL_OPERATORS = ["level", "levelize", "gamma", "negate", "sigmoidal", "auto_level", "linear_stretch", "normalize",
                   "brightness_contrast", "min_max_stretch"]
SCALE_OPERATORS = ["sample", "scale", "thumbnail"]


def statistic_fits(statistic, width, height, is_float):
    """launch_statistic's LDS limit: the staged window of one channel."""
    element = 2 if statistic in statistic_oracle.RANK or not is_float else 4
    return (max(width, 1) + 15) * (max(height, 1) + 15) * element <= 65536


def sample_offsets_fit(source, destination, percent):
    """SampleImage's offset table stays inside the frame (the library declines the rest: the reference then reads
    virtual pixels)."""
    return int(scale_oracle.sample_offsets(source, destination, percent).max()) < source


def new_case(op, layouts):
    """What every case of families 19 to 25 draws first: the Quantum type, the precision mode, the memory kind, the layout and
    the alpha kind of pixels / float_pixels."""
    layout = layouts[int(rng.integers(0, len(layouts)))]
    drawn[op] = drawn.get(op, 0) + 1
    return {"op": op, "index": drawn[op] - 1, "float": bool(rng.random() < 0.5), "fast": bool(rng.random() < 0.5),
            "host": bool(rng.random() < 0.2), "layout": layout, "channels": LAYOUT_CHANNELS[layout],
            "kind": int(rng.integers(0, 6)), "mask": None, "copy": (), "bits": None, "colorspace": "sRGB", "intensity": None,
            "source": "kind"}


def draw_mask(case):
    """A channel mask in half the cases, drawn as family 16 draws it (four plain channels keep the default mask, as in the
    operators' own tests); the channels left out are copy channels."""
    if case["layout"] != "plain4" and rng.random() < 0.5:
        channels = case["channels"]
        letters = MASK_LETTERS[channels]
        keep = [c for c in range(channels) if rng.random() < 0.5] or [int(rng.integers(0, channels))]
        case.update(mask="".join(letters[c] for c in keep), copy=tuple(c for c in range(channels) if c not in keep),
                    bits=sum(MASK_BITS[letters[c]] for c in keep))


def draw_sides(most_rows, most_cols):
    """Frame sides from 1 up; one case in five is thin (one side 1 to 3)."""
    rows, cols = int(rng.integers(1, most_rows + 1)), int(rng.integers(1, most_cols + 1))
    if rng.random() < 0.2:
        thin = int(rng.integers(1, 4))
        rows, cols = (thin, cols) if rng.random() < 0.5 else (rows, thin)
    return rows, cols


def shrink_to_work(rows, cols, per_pixel, most):
    """Halves the longer side until rows x cols x per_pixel fits `most`."""
    while rows * cols * per_pixel > most and max(rows, cols) > 1:
        rows, cols = (max(rows // 2, 1), cols) if rows >= cols else (rows, max(cols // 2, 1))
    return rows, cols


def new_seed():
    return int(rng.integers(0, 1 << 30))


def smooth_frame(rows, cols, channels, is_float):
    """A ramp of 300 levels a column and 150 a row under 400 levels of noise: a SelectiveBlurImage threshold splits its windows."""
    y, x = np.mgrid[0:rows, 0:cols]
    base = (x * 300.0 + y * 150.0) % 60000.0
    a = np.stack([base * (0.6 + 0.1 * c) + rng.integers(0, 400, (rows, cols)) for c in range(channels)], axis=2)
    if is_float:
        return np.ascontiguousarray((a + rng.random(a.shape)).astype(np.float32))
    return np.ascontiguousarray(a.astype(np.uint16))


def all_pixels_gray(frame):
    """IsPixelGray (pixel-accessor.h:561-578) on every pixel of a frame with three colour channels."""
    if frame.shape[2] < 3:
        return False
    p = frame[..., :3].astype(np.float64)
    return bool(((np.abs(p[..., 0] - p[..., 1]) < 1.0e-12) & (np.abs(p[..., 1] - p[..., 2]) < 1.0e-12)).all())


def gamma_draw():
    """0, 1, or log-uniform over 0.1 ... 10."""
    u = rng.random()
    return 0.0 if u < 0.15 else 1.0 if u < 0.4 else float(10.0 ** rng.uniform(-1.0, 1.0))


def draw_statistic_case(op=19):
    case = new_case(op, ["gray", "gray+alpha", "rgb", "rgba"])
    is_float, channels = case["float"], case["channels"]
    while True:
        statistic = list(statistic_oracle.TYPES)[int(rng.integers(0, len(statistic_oracle.TYPES)))]
        u = rng.random()
        if case["index"] % 3 == 0:
            statistic = statistic_oracle.RANK[int(rng.integers(0, 3))]
            width, height = STATISTIC_ROUTE_WINDOWS[(case["index"] // 3) % len(STATISTIC_ROUTE_WINDOWS)]
        elif u < 0.05:                                 # up to the LDS limit: one side long, the other what still fits
            width = int(rng.integers(41, 400))
            height = int(rng.integers(1, max(2, 32768 // (width + 15) - 14)))
            if rng.random() < 0.5:
                width, height = height, width
        elif u < 0.05 + 1.0 / 6.0:
            width, height = int(rng.integers(13, 41)), int(rng.integers(13, 41))
        else:
            width, height = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        if statistic_fits(statistic, width, height, is_float):
            break
    rows, cols = shrink_to_work(*draw_sides(120, 160), channels * max(width, 1) * max(height, 1), STATISTIC_WORK)
    if statistic in statistic_oracle.RANK and rng.random() < 1.0 / 3.0:
        keys, seed = ["binary", "levels"][int(rng.integers(0, 2))], new_seed()
        frame = statistic_oracle.repeated_keys(rows, cols, channels, np.float32 if is_float else np.uint16, keys, seed)
        case["source"] = "repeated_keys %s seed %d" % (keys, seed)
    else:
        frame = enhance_frame(rows, cols, channels, is_float, case["kind"])
        if is_float:
            if rng.random() < 1.0 / 3.0:
                frame = rng.uniform(-3000.0, 70000.0, frame.shape).astype(np.float32)
                case["source"] = "uniform -3000 ... 70000"
            frame[rng.random(frame.shape) < 0.01] = np.nan
    draw_mask(case)
    case.update(name="statistic", args=(statistic, width, height), frame=np.ascontiguousarray(frame))
    return case


def draw_edge_blur_case(op=20):
    case = new_case(op, ["gray", "gray+alpha", "rgb", "rgba"])
    is_float, channels = case["float"], case["channels"]
    dtype = np.float32 if is_float else np.uint16
    if rng.random() < 0.5:
        def side():                                    # odd, 0 meaning 1
            u = rng.random()
            return 0 if u < 0.1 else 2 * int(rng.integers(0, 8 if u > 0.1 + 1.0 / 6.0 else 17)) + 1
        width, height = side(), side()
        rows, cols = shrink_to_work(*draw_sides(100, 140), channels * max(width, 1) * max(height, 1), EDGE_BLUR_WORK)
        high, seed = (70000 if is_float and rng.random() < 1.0 / 3.0 else 65535), new_seed()
        # samples from 300 up only: the reference never writes the table slot a zero intensity byte reads (edge_blur_oracle)
        frame = edge_blur_oracle.bilateral_pixels(rows, cols, channels, dtype, seed=seed, high=high)
        case.update(name="bilateral_blur", args=(width, height, float(rng.uniform(1.0, 250.0)), float(rng.uniform(0.5, 12.0))),
                    source="bilateral_pixels seed %d high %d" % (seed, high))
    else:
        if rng.random() < 0.5:
            radius, sigma = 0.0, float(rng.uniform(0.5, 4.0))
            reach = 8.0 * sigma + 3.0                  # no narrower than the width the reference takes from the sigma
        else:
            radius, sigma = float(rng.integers(1, 7)), float(rng.uniform(0.5, 4.0))
            reach = 2.0 * radius + 1.0
        u = rng.random()
        threshold = 0.0 if u < 0.1 else 1e9 if u < 0.2 else float(10.0 ** rng.uniform(0.0, 5.0))
        rows, cols = shrink_to_work(*draw_sides(100, 140), channels * reach * reach, EDGE_BLUR_WORK)
        if rng.random() < 0.5:
            frame = smooth_frame(rows, cols, channels, is_float)
            if channels in (2, 4):                     # ... with the alpha of the drawn kind, a sprite's included
                frame[..., -1] = enhance_frame(rows, cols, 4, is_float, case["kind"])[..., 3]
            case["source"] = "smooth"
        else:
            frame = enhance_frame(rows, cols, channels, is_float, case["kind"])
        if channels >= 3:
            case.update(intensity=SELECTIVE_INTENSITIES[int(rng.integers(0, len(SELECTIVE_INTENSITIES)))],
                        colorspace=["sRGB", "RGB"][int(rng.integers(0, 2))])
        case.update(name="selective_blur", args=(radius, sigma, threshold))
    draw_mask(case)
    case["frame"] = np.ascontiguousarray(frame)
    return case


def draw_kuwahara_case(op=21):
    case = new_case(op, kuwahara_oracle.LAYOUTS)
    is_float, channels = case["float"], case["channels"]
    radius = float(rng.integers(8, 16)) if rng.random() < 0.1 else float(KUWAHARA_RADII[int(rng.integers(0, len(KUWAHARA_RADII)))])
    rows, cols = draw_sides(100, 140)
    frame = enhance_frame(rows, cols, channels, is_float, case["kind"])
    if is_float and rng.random() < 1.0 / 3.0:
        which, seed = ["wide_range_float", "out_of_range_float"][int(rng.integers(0, 2))], new_seed()
        frame = getattr(kuwahara_oracle, which)(rows, cols, channels, seed=seed)
        case["source"] = "%s seed %d" % (which, seed)
    if case["layout"] in ("gray+alpha", "rgba") and rng.random() < 1.0 / 3.0:
        seed = new_seed()
        frame = kuwahara_oracle.sprite_alpha(frame, fraction=0.6, seed=seed)
        case["source"] += " sprite_alpha seed %d" % seed
    draw_mask(case)
    case.update(name="kuwahara", args=(radius, float(rng.uniform(0.3, 3.5))), frame=np.ascontiguousarray(frame))
    return case


def draw_clahe_case(op=22):
    case = new_case(op, ["rgb", "rgba"])
    is_float, channels = case["float"], case["channels"]
    dtype = np.float32 if is_float else np.uint16
    rows, cols = int(rng.integers(16, 201)), int(rng.integers(16, 261))      # (automatic tiles are an eighth of a side)
    while True:
        width, height = (0 if rng.random() < 0.2 else int(rng.integers(2, 65)) for _ in range(2))
        bins = CLAHE_BINS[int(rng.integers(0, len(CLAHE_BINS)))]
        if clahe_oracle.table_fits(rows, cols, channels, dtype, width, height, bins):
            break
    clip = CLAHE_CLIPS[int(rng.integers(0, len(CLAHE_CLIPS)))] if rng.random() < 0.5 else float(rng.uniform(0.1, 8.0))
    # Q16: the whole operator from sRGB or the core on a frame declared Lab; float Quantum: the core only (from sRGB the
    # contract is "equals the device's own chain", README: CLAHEImage, and stays with test_gpu_clahe.py)
    case["colorspace"] = "Lab" if is_float or rng.random() < 0.5 else "sRGB"
    u = rng.random()
    if is_float and u < 0.25:
        seed = new_seed()
        frame, case["source"] = clahe_oracle.float_specials(rows, cols, channels, seed=seed), "float_specials seed %d" % seed
    elif u < 0.6:
        which = sorted(clahe_oracle.INPUTS)[int(rng.integers(0, len(clahe_oracle.INPUTS)))]
        frame, case["source"] = clahe_oracle.INPUTS[which](rows, cols, channels, dtype), which
    else:
        frame = enhance_frame(rows, cols, channels, is_float, case["kind"])
    draw_mask(case)
    case.update(name="clahe", args=(width, height, bins, clip), frame=np.ascontiguousarray(frame))
    return case


def draw_threshold_case(op=23):
    case = new_case(op, threshold_oracle.LAYOUTS)
    which = THRESHOLD_OPERATORS[case["index"] % len(THRESHOLD_OPERATORS)]      # equal shares
    if which in ("black", "white", "range") and case["layout"] not in COLOUR_LAYOUTS:
        case["layout"] = COLOUR_LAYOUTS[int(rng.integers(0, len(COLOUR_LAYOUTS)))]
    if which in ("bilevel", "auto") and rng.random() < 0.35:      # an intensity method of its own, on a colour frame
        names = list(threshold_oracle.INTENSITIES)
        case.update(intensity=names[int(rng.integers(0, len(names)))], colorspace=["sRGB", "RGB"][int(rng.integers(0, 2))],
                    layout=["rgb", "rgba"][int(rng.integers(0, 2))])
    case["channels"] = LAYOUT_CHANNELS[case["layout"]]
    channels = case["channels"]
    if which == "adaptive":
        ordinal = case["index"] // len(THRESHOLD_OPERATORS)
        shape = {1: "strip", 3: "band"}.get(ordinal % 10, "plain")      # one adaptive case in ten each, on Q16
        if shape != "plain":
            case["float"] = False
        is_float = case["float"]
        width = int(rng.integers(41, ADAPTIVE_MAX_WIDTH + 1)) if not is_float and rng.random() < 0.125 else int(rng.integers(0, 41))
        height = int(rng.integers(41, 151)) if rng.random() < 0.125 else int(rng.integers(0, 41))
        rows, cols = draw_sides(140, 200)
        if shape == "strip":                           # more columns than one strip keeps: 512-(W-1)
            rows, cols = min(rows, 24), ADAPTIVE_SPAN - (max(width, 1) - 1) + int(rng.integers(1, 60))
        elif shape == "band":                          # more rows than one band: max(64, 4H)
            rows, cols = max(ADAPTIVE_BAND_ROWS, 4 * height) + int(rng.integers(1, 40)), min(cols, 40)
        bias = float(ADAPTIVE_BIASES[int(rng.integers(0, len(ADAPTIVE_BIASES)))]) if rng.random() < 0.5 else float(rng.uniform(-3000.0, 3000.0))
        if is_float and rng.random() < 1.0 / 3.0:      # the running sum carries its rounding along the row
            seed = new_seed()
            frame, case["source"] = kuwahara_oracle.wide_range_float(rows, cols, channels, seed=seed), "wide_range_float seed %d" % seed
        else:
            frame = enhance_frame(rows, cols, channels, is_float, case["kind"])
        case.update(name="adaptive", args=(width, height, bias), shape=shape)
    else:
        is_float = case["float"]
        dtype = np.float32 if is_float else np.uint16
        rows, cols = draw_sides(140, 200)
        u = rng.random()
        if u < 0.125:
            frame, case["source"] = threshold_oracle.constant(rows, cols, channels, dtype), "constant"
        elif u < 0.25:
            seed = new_seed()
            frame, case["source"] = threshold_oracle.two_level(rows, cols, channels, dtype, seed=seed), "two_level seed %d" % seed
        else:
            frame = enhance_frame(rows, cols, channels, is_float, case["kind"])

        def level():                                   # a quarter exactly on a sample of the frame: the < / <= edges
            if rng.random() < 0.25:
                return float(frame[int(rng.integers(0, rows)), int(rng.integers(0, cols)), int(rng.integers(0, channels))])
            return float(rng.uniform(-1000.0, 67000.0))
        if which == "bilevel":
            args = (level(),)
        elif which in ("black", "white"):
            args = (tuple(level() for _ in range(channels)),)
        elif which == "range":
            args = tuple(sorted(level() for _ in range(4)))
        else:
            args = (list(threshold_oracle.METHODS)[int(rng.integers(0, len(threshold_oracle.METHODS)))],)
        case.update(name=which, args=args)
    draw_mask(case)
    case["frame"] = np.ascontiguousarray(frame)
    return case


def draw_levels_case(op=24):
    case = new_case(op, levels_oracle.LAYOUTS)
    is_float, channels = case["float"], case["channels"]
    which = LEVEL_OPERATORS[int(rng.integers(0, len(LEVEL_OPERATORS)))]
    while True:
        rows, cols = draw_sides(200, 260)
        frame = enhance_frame(rows, cols, channels, is_float, case["kind"])
        case["source"] = "kind"
        if which in ("auto_level", "normalize", "min_max_stretch", "linear_stretch") and rng.random() < 0.5:
            low, span = float(rng.uniform(0.0, 30000.0)), float(rng.uniform(0.0, 0.5))      # a range for the stretch to find
            frame = (frame * span + low).astype(frame.dtype) if is_float else (frame * span + low).astype(np.uint16)
            case["source"] = "kind x %.17g + %.17g" % (span, low)
        if channels >= 3 and rng.random() < 0.25:
            seed = new_seed()
            frame = levels_oracle.gray_pixels(frame, seed=seed)
            case["source"] += " gray_pixels seed %d" % seed
        if which != "normalize" or not all_pixels_gray(frame):
            break
        # NormalizeImage is ContrastStretchImage, which hands a colour frame that IdentifyImageType would call gray back
        # untouched (MagickHipContrastStretchImage, enhance.c:1586: the reference re-lays it out): another frame, another kind
        case["kind"] = (case["kind"] + 1) % 6
    libm = False
    if which in ("level", "levelize"):
        gamma = gamma_draw()
        args = (float(rng.uniform(-5000.0, 70000.0)), float(rng.uniform(-5000.0, 70000.0)), gamma)
        libm = level_libm(gamma) if which == "level" else gamma != 1.0
    elif which == "gamma":
        args = (gamma_draw(),)
    elif which == "negate":
        args = (bool(rng.random() < 0.5),)
    elif which == "sigmoidal":
        args, libm = (bool(rng.random() < 0.5), float(10.0 ** rng.uniform(-2.0, np.log10(20.0))), float(rng.uniform(-1000.0, 70000.0))), True
    elif which == "linear_stretch":
        args = (float(rng.uniform(0.0, rows * cols)), float(rng.uniform(0.0, rows * cols)))
    elif which == "brightness_contrast":
        args = (float(rng.uniform(-100.0, 100.0)), float(rng.uniform(-100.0, 100.0)))
    elif which == "min_max_stretch":
        gamma = gamma_draw()
        args, libm = (float(rng.uniform(0.0, 2000.0)), float(rng.uniform(0.0, 2000.0)), gamma), gamma != 1.0
    else:
        args = ()
    draw_mask(case)
    case.update(name=which, args=args, libm=libm, frame=np.ascontiguousarray(frame))
    return case


def draw_scale_case(op=25):
    case = new_case(op, scale_oracle.LAYOUTS)
    which = SCALE_OPERATORS[int(rng.integers(0, len(SCALE_OPERATORS)))]
    if which == "thumbnail" and case["layout"] not in ("rgb", "rgba"):      # the layouts test_thumbnail runs
        case["layout"] = ["rgb", "rgba"][int(rng.integers(0, 2))]
        case["channels"] = LAYOUT_CHANNELS[case["layout"]]
    is_float, channels = case["float"], case["channels"]
    dtype = np.float32 if is_float else np.uint16
    offset = scale_oracle.SAMPLE_OFFSETS[int(rng.integers(0, len(scale_oracle.SAMPLE_OFFSETS)))] if which == "sample" else None
    while True:
        rows, cols = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        if rng.random() < 1.0 / 6.0:
            rows, cols = (1, cols) if rng.random() < 0.5 else (rows, 1)
        to_rows, to_cols = int(rng.integers(1, 401)), int(rng.integers(1, 401))
        u = rng.random()
        if u < 0.1:                                    # an integer factor exactly, either way
            rows, cols = min(rows, 75), min(cols, 75)
            fy, fx = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            if rng.random() < 0.5:
                to_rows, to_cols = rows * fy, cols * fx
            else:
                to_rows, to_cols, rows, cols = rows, cols, rows * fy, cols * fx
        elif u < 0.2:                                  # source and destination coprime
            while np.gcd(rows, to_rows) != 1:
                to_rows = to_rows % 400 + 1
            while np.gcd(cols, to_cols) != 1:
                to_cols = to_cols % 400 + 1
        ox, oy = scale_oracle.offset_percent(offset)
        if which != "sample" or (rows, cols) == (to_rows, to_cols) or \
                (sample_offsets_fit(rows, to_rows, oy) and sample_offsets_fit(cols, to_cols, ox)):
            break
    transparent = [0.0, 0.2, 0.9][int(rng.integers(0, 3))]
    seed = new_seed()
    if is_float and scale_oracle.layout_has_alpha(case["layout"]) and rng.random() < 0.25:
        frame, case["source"] = scale_oracle.negative_alpha_float(rows, cols, channels, seed=seed), "negative_alpha_float seed %d" % seed
    else:
        frame = scale_oracle.frame(case["layout"], rows, cols, dtype, seed=seed, transparent=transparent)
        case["source"] = "frame seed %d transparent %g" % (seed, transparent)
    draw_mask(case)
    case.update(name=which, args=(to_rows, to_cols), offset=offset, frame=np.ascontiguousarray(frame))
    return case


DRAWS = {19: draw_statistic_case, 20: draw_edge_blur_case, 21: draw_kuwahara_case, 22: draw_clahe_case,
         23: draw_threshold_case, 24: draw_levels_case, 25: draw_scale_case}


def case_image(case, frame=None):
    """The case's frame (a fresh copy: some operators work in place) as the library sees it."""
    frame = case["frame"] if frame is None else frame
    kw = {"colorspace": case["colorspace"], "has_alpha": case["layout"] in ("gray+alpha", "rgba"), "copy_channels": case["copy"]}
    if case["bits"] is not None:
        kw["channel_mask"] = case["bits"]
    if case["intensity"] is not None:
        kw["intensity"] = threshold_oracle.INTENSITIES[case["intensity"]]
    if case["host"]:
        return im.Image(frame.copy(), **kw)
    return (dev_float if case["float"] else dev)(frame, **kw)


def case_reference(case):
    return threshold_oracle.ref_image(refmod, case["frame"], case["colorspace"], mask=case["mask"], intensity=case["intensity"])


def describe(case):
    frame = case["frame"]
    return "#%d %s %s %dx%dx%d %s kind %d (%s) mask %s %s intensity %s %s %s" % (
        case["index"], case["args"], frame.dtype.name, frame.shape[0], frame.shape[1], frame.shape[2], case["layout"], case["kind"],
        case["source"], case["mask"], case["colorspace"], case["intensity"], "fast" if case["fast"] else "exact",
        "host" if case["host"] else "device")


def compare(name, got, want, what, libm=False, ulp=0, level=0):
    """Bit-identical (float NaNs at the same places); ulp, level: what a float / a Q16 sample may be off; libm: float within
    one ULP and, from 10 000 samples on, at most LIBM_SHARE of them different at all (test_gpu_levels.py)."""
    if got.shape != want.shape:
        print("MISMATCH %s %s: shape %s, reference %s" % (name, what, got.shape, want.shape), flush=True)
        return 1
    if want.dtype != np.float32:
        return check(name, got, want, level, what)
    if not libm:
        return check_ulp(name, got, want, ulp, what) if ulp else check_bits(name, got, want, what)
    if check_ulp(name, got, want, 1, what):
        return 1
    differ = ~((got.view(np.uint32) == want.view(np.uint32)) | np.isnan(want))
    if want.size >= 10000 and differ.mean() > LIBM_SHARE:
        print("MISMATCH %s %s: %.3g of the samples differ (at most %g)" % (name, what, differ.mean(), LIBM_SHARE), flush=True)
        return 1
    return 0


def run_statistic(case, what):
    got = im.statistic_image(case_image(case), *case["args"]).numpy()
    want = statistic_oracle.ref_statistic(refmod, case_reference(case), *case["args"]).numpy()
    return compare("statistic", got, want, what)


def run_edge_blur(case, what):
    if case["name"] == "bilateral_blur":
        got = im.bilateral_blur_image(case_image(case), *case["args"]).numpy()
        want = edge_blur_oracle.ref_bilateral(refmod, case_reference(case), *case["args"]).numpy()
    else:
        got = im.selective_blur_image(case_image(case), *case["args"]).numpy()
        want = edge_blur_oracle.ref_selective(refmod, case_reference(case), *case["args"]).numpy()
    return compare(case["name"], got, want, what)


def run_kuwahara(case, what):
    got = im.kuwahara_image(case_image(case), *case["args"]).numpy()
    if case["layout"] == "plain4":
        want = kuwahara_oracle.plain4_reference(refmod, case["frame"], *case["args"])
    else:
        want = kuwahara_oracle.ref_kuwahara(refmod, case_reference(case), *case["args"]).numpy()
    return compare("kuwahara", got, want, what)


def run_clahe(case, what):
    got = im.clahe_image(case_image(case), *case["args"]).numpy()
    want = clahe_oracle.ref_clahe(case_reference(case), *case["args"]).numpy()
    return compare("clahe", got, want, what)


def run_threshold(case, what):
    name, args, image, ref = case["name"], case["args"], case_image(case), case_reference(case)
    if name == "adaptive":
        got = im.adaptive_threshold_image(image, *args).numpy()
        want = threshold_oracle.ref_adaptive_threshold(refmod, ref, *args).numpy()
    elif name == "bilevel":
        got, want = im.bilevel_image(image, *args).numpy(), threshold_oracle.ref_bilevel(ref, *args).numpy()
    elif name == "black":
        got, want = im.black_threshold_image(image, args[0]).numpy(), threshold_oracle.ref_black_threshold(ref, args[0]).numpy()
    elif name == "white":
        got, want = im.white_threshold_image(image, args[0]).numpy(), threshold_oracle.ref_white_threshold(ref, args[0]).numpy()
    elif name == "range":
        got, want = im.range_threshold_image(image, *args).numpy(), threshold_oracle.ref_range_threshold(ref, *args).numpy()
    else:
        image, percent = im.auto_threshold_image(image, args[0])
        ref, text = threshold_oracle.ref_auto_threshold(ref, args[0])
        if "%g%%" % percent != text:
            print("MISMATCH auto %s: threshold %g%%, reference %s" % (what, percent, text), flush=True)
            return 1
        got, want = image.numpy(), ref.numpy()
    return compare(name, got, want, what)


def run_levels(case, what):
    name, args, image, ref = case["name"], case["args"], case_image(case), case_reference(case)
    if name == "auto_level":
        measured, expected = im.image_range(case_image(case)), levels_oracle.ref_range(case_reference(case))
        if measured != expected:
            print("MISMATCH auto_level %s: range %r, reference %r" % (what, measured, expected), flush=True)
            return 1
    if name == "linear_stretch":
        image, black, white = im.linear_stretch_image(image, *args)
        ref, text = levels_oracle.ref_linear_stretch(ref, *args)
        if levels_oracle.linear_stretch_property(black, white) != text:
            print("MISMATCH linear_stretch %s: bins %d, %d, reference %s" % (what, black, white, text), flush=True)
            return 1
    else:
        image = {"level": im.level_image, "levelize": im.levelize_image, "gamma": im.gamma_image, "negate": im.negate_image,
                 "sigmoidal": im.sigmoidal_contrast_image, "auto_level": im.auto_level_image, "normalize": im.normalize_image,
                 "brightness_contrast": im.brightness_contrast_image, "min_max_stretch": im.min_max_stretch_image}[name](image, *args)
        ref = {"level": levels_oracle.ref_level, "levelize": levels_oracle.ref_levelize, "gamma": levels_oracle.ref_gamma,
               "negate": levels_oracle.ref_negate, "sigmoidal": levels_oracle.ref_sigmoidal, "auto_level": levels_oracle.ref_auto_level,
               "normalize": levels_oracle.ref_normalize, "brightness_contrast": levels_oracle.ref_brightness_contrast,
               "min_max_stretch": levels_oracle.ref_min_max_stretch}[name](ref, *args)
    return compare(name, image.numpy(), ref.numpy(), what, libm=case["libm"])


def run_scale(case, what):
    name, (to_rows, to_cols), image, ref = case["name"], case["args"], case_image(case), case_reference(case)
    what += " sample:offset %s" % case["offset"]
    if name == "sample":
        got = im.sample_image(image, to_cols, to_rows, None if case["offset"] is None else scale_oracle.offset_percent(case["offset"])).numpy()
        want = scale_oracle.ref_sample(refmod, ref, to_rows, to_cols, case["offset"]).numpy()
    elif name == "scale":
        got, want = im.scale_image(image, to_cols, to_rows).numpy(), scale_oracle.ref_scale(refmod, ref, to_rows, to_cols).numpy()
    else:
        # ThumbnailImage keeps ResizeImage's contract: FAST within one level / one float ULP (test_gpu_scale.py, test_thumbnail)
        got, want = im.thumbnail_image(image, to_cols, to_rows).numpy(), scale_oracle.ref_thumbnail(refmod, ref, to_rows, to_cols).numpy()
        return compare(name, got, want, what, ulp=1 if case["fast"] else 0, level=1 if case["fast"] else 0)
    return compare(name, got, want, what)


RUNS = {19: run_statistic, 20: run_edge_blur, 21: run_kuwahara, 22: run_clahe, 23: run_threshold, 24: run_levels, 25: run_scale}


def run_domain_case(case):
    """Families 19 to 25 against the compiled reference, in the case's precision mode (restored afterwards)."""
    what = describe(case)
    im.set_precision(im.PRECISION_FAST if case["fast"] else im.PRECISION_EXACT)
    try:
        return RUNS[case["op"]](case, what)
    except im.MagickHipError as error:
        print("MISMATCH %s %s: declined inside the stated domain (%s)" % (case["name"], what, error), flush=True)
        return 1
    finally:
        im.set_precision(im.PRECISION_EXACT)


def run_case(op=None):
    """One random case of operator family `op` (None: any); returns the number of mismatches (0 or 1)."""
    failures = 0
    if op is not None and op >= 19:                # (their draws start at the seed: test_stress_draws.py sees the same cases)
        return run_domain_case(DRAWS[op](op))
    rows, cols, kind, px = draw_frame()
    if op is None:
        op = int(rng.integers(0, NUMBER_OF_OPS))
    if op >= 19:
        return run_domain_case(DRAWS[op](op))
    if op >= 16:
        return run_enhance_case(draw_enhance_case(op))
    detail = "%dx%d kind %d" % (rows, cols, kind)
    ref = refmod.RefImage(px)
    if op == 0:                                    # FAST blur, every kernel length of the fused launch
        sigma = float(rng.uniform(0.3, 13.4))
        radius = blur_radius(sigma)
        im.set_precision(im.PRECISION_FAST)
        got = im.blur_image(dev(px), radius, sigma).numpy()
        im.set_precision(im.PRECISION_EXACT)
        failures += check("fast blur", got, ref.blur(radius, sigma).numpy(), 1, detail + " %gx%.3f" % (radius, sigma))
    elif op == 1:                                  # EXACT blur (Tie64)
        sigma = float(rng.uniform(0.3, 13.4))
        radius = blur_radius(sigma)
        got = im.blur_image(dev(px), radius, sigma).numpy()
        failures += check("exact blur", got, ref.blur(radius, sigma).numpy(), 0, detail + " %gx%.3f" % (radius, sigma))
    elif op == 2:                                  # FAST unsharp in the fused launch
        sigma = float(rng.uniform(0.5, 12.0))
        gain, threshold = float(rng.uniform(0.3, 3.0)), float(rng.uniform(0.0, 0.2))
        radius = blur_radius(sigma)
        im.set_precision(im.PRECISION_FAST)
        got = im.unsharp_mask_image(dev(px), radius, sigma, gain, threshold).numpy()
        im.set_precision(im.PRECISION_EXACT)
        want = ref.unsharp(radius, sigma, gain, threshold).numpy()
        blurred = ref.blur(radius, sigma).numpy().astype(np.int64)
        edge = np.abs(2 * np.abs(px.astype(np.int64) - blurred) - 65535.0 * threshold) <= 2.0
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        d[edge] = 0
        failures += check("fast unsharp", d, np.zeros_like(d), int(np.ceil(1.0 + gain)),
                          detail + " %gx%.3f gain %.2f thr %.3f" % (radius, sigma, gain, threshold))
    elif op == 3:                                  # symmetric convex kernels (rects)
        family = ["Disk:%.1f" % rng.uniform(0.5, 16.0), "Square:%d" % rng.integers(1, 9),
                  "Diamond:%d" % rng.integers(1, 12), "Octagon:%d" % rng.integers(1, 10),
                  "Plus:%d" % rng.integers(1, 12), "Rectangle:%dx%d" % (2 * rng.integers(0, 9) + 1, 2 * rng.integers(0, 9) + 1)]
        kernel = family[int(rng.integers(0, len(family)))]
        method = "Dilate" if rng.random() < 0.5 else "Erode"
        layout = int(rng.integers(0, 3))           # RGBA; one channel (four row bands); RGB (a fourth, empty channel)
        if layout == 0:
            got = im.morphology_image(dev(px), method, 1, kernel).numpy()
            failures += check(method, got, ref.morphology(method, 1, kernel).numpy(), 0, detail + " " + kernel)
        else:
            frame = np.ascontiguousarray(px[:, :, :1] if layout == 1 else px[:, :, :3])
            iterations = 1 if rng.random() < 0.8 else int(rng.integers(2, 4))
            got = im.morphology_image(dev(frame), method, iterations, kernel).numpy().reshape(frame.shape)
            want = refmod.RefImage(frame).morphology(method, iterations, kernel).numpy().reshape(frame.shape)
            failures += check(method, got, want, 0, detail + " %s x%d c%d" % (kernel, iterations, frame.shape[2]))
    elif op == 4:                                  # histogram operators above a megapixel
        rows2, cols2 = int(rng.integers(1000, 1500)), int(rng.integers(1050, 1900))
        px2 = pixels(rows2, cols2, int(rng.integers(0, 4)))
        px2[0, 0] = (1, 2, 3, 4)
        n = rows2 * cols2
        black, white = float(rng.uniform(0, 0.1)) * n, n - float(rng.uniform(0, 0.1)) * n
        if rng.random() < 0.5:
            got = im.contrast_stretch_image(dev(px2), black, white).numpy()
            want = refmod.RefImage(px2).contrast_stretch(black, white).numpy()
        else:
            got = im.equalize_image(dev(px2)).numpy()
            want = refmod.RefImage(px2).equalize().numpy()
        failures += check("histogram op", got, want, 0, "%dx%d" % (rows2, cols2))
    elif op == 5:                                  # FAST 2-D convolve on the matrix cores
        family = ["Disk:%.1f" % rng.uniform(2.0, 15.9), "Octagon:%d" % rng.integers(2, 12),
                  "Diamond:%d" % rng.integers(2, 14), "Plus:%d" % rng.integers(2, 14),
                  "Ring:%d,%d" % (rng.integers(2, 6), rng.integers(7, 15))]
        kernel = family[int(rng.integers(0, len(family)))]
        layout = int(rng.integers(0, 4))           # RGBA three times in four; one channel (four row bands); RGB
        frame = px if layout < 2 else np.ascontiguousarray(px[:, :, :1] if layout == 2 else px[:, :, :3])
        im.set_precision(im.PRECISION_FAST)
        got = im.morphology_image(dev(frame), "Convolve", 1, kernel, scale=(1.0, 1)).numpy().reshape(frame.shape)
        im.set_precision(im.PRECISION_EXACT)
        want = (ref if layout < 2 else refmod.RefImage(frame)).set_artifact("convolve:scale", "!") \
            .morphology("Convolve", 1, kernel).numpy().reshape(frame.shape)
        failures += check("fast convolve 2-D", got, want, 1, detail + " %s c%d" % (kernel, frame.shape[2]))
    elif op == 7:                                  # EXACT 2-D separable kernels (+ the odd centre cell)
        sigma = float(rng.uniform(0.8, 4.5))
        if rng.random() < 0.6:
            got = im.gaussian_blur_image(dev(px), 0.0, sigma).numpy()
            failures += check("exact gaussian", got, ref.gaussian_blur(0.0, sigma).numpy(), 0, detail + " sigma %.3f" % sigma)
        else:
            got = im.sharpen_image(dev(px), 0.0, sigma).numpy()
            failures += check("exact sharpen", got, ref.sharpen(0.0, sigma).numpy(), 0, detail + " sigma %.3f" % sigma)
    elif op == 8:                                  # float Quantum: blur / unsharp on the fp64 kernels
        fpx = float_pixels(rows, cols, kind)
        fref = refmod.RefImage(fpx)
        sigma = float(rng.uniform(0.5, 12.0))
        radius = blur_radius(sigma)
        if rng.random() < 0.5:
            got = im.blur_image(dev_float(fpx), radius, sigma).numpy()
            failures += check_bits("float blur", got, fref.blur(radius, sigma).numpy(), detail + " %gx%.3f" % (radius, sigma))
        else:
            gain, threshold = float(rng.uniform(0.3, 3.0)), float(rng.uniform(0.0, 0.2))
            got = im.unsharp_mask_image(dev_float(fpx), radius, sigma, gain, threshold).numpy()
            failures += check_bits("float unsharp", got, fref.unsharp(radius, sigma, gain, threshold).numpy(),
                                   detail + " %gx%.3f gain %.2f thr %.3f" % (radius, sigma, gain, threshold))
    elif op == 9:                                  # float Quantum: union-of-rectangles Erode / Dilate
        fpx = float_pixels(rows, cols, kind)
        family = ["Disk:%.1f" % rng.uniform(0.5, 16.0), "Square:%d" % rng.integers(1, 9),
                  "Diamond:%d" % rng.integers(1, 12), "Octagon:%d" % rng.integers(1, 10),
                  "Rectangle:%dx%d" % (2 * rng.integers(0, 9) + 1, 2 * rng.integers(0, 9) + 1)]
        kernel = family[int(rng.integers(0, len(family)))]
        method = "Dilate" if rng.random() < 0.5 else "Erode"
        if rng.random() < 0.4:                     # RGB: a fourth, empty channel
            fpx = np.ascontiguousarray(fpx[:, :, :3])
        got = im.morphology_image(dev_float(fpx), method, 1, kernel).numpy().reshape(fpx.shape)
        failures += check_bits("float " + method, got, refmod.RefImage(fpx).morphology(method, 1, kernel).numpy().reshape(fpx.shape),
                               detail + " %s c%d" % (kernel, fpx.shape[2]))
    elif op == 10:                                 # float Quantum: separable 2-D kernels
        fpx = float_pixels(rows, cols, kind)
        sigma = float(rng.uniform(0.8, 4.5))
        if rng.random() < 0.6:
            got = im.gaussian_blur_image(dev_float(fpx), 0.0, sigma).numpy()
            failures += check_bits("float gaussian", got, refmod.RefImage(fpx).gaussian_blur(0.0, sigma).numpy(),
                                   detail + " sigma %.3f" % sigma)
        else:
            got = im.sharpen_image(dev_float(fpx), 0.0, sigma).numpy()
            failures += check_bits("float sharpen", got, refmod.RefImage(fpx).sharpen(0.0, sigma).numpy(),
                                   detail + " sigma %.3f" % sigma)
    elif op == 11:                                 # float Quantum: histogram operators above a megapixel
        rows2, cols2 = int(rng.integers(1000, 1400)), int(rng.integers(1050, 1500))
        fpx = float_pixels(rows2, cols2, int(rng.integers(0, 2)))
        n = rows2 * cols2
        black, white = float(rng.uniform(0, 0.1)) * n, n - float(rng.uniform(0, 0.1)) * n
        if rng.random() < 0.5:
            got = im.contrast_stretch_image(dev_float(fpx), black, white).numpy()
            want = refmod.RefImage(fpx).contrast_stretch(black, white).numpy()
        else:
            got = im.equalize_image(dev_float(fpx)).numpy()
            want = refmod.RefImage(fpx).equalize().numpy()
        failures += check_bits("float histogram op", got, want, "%dx%d" % (rows2, cols2))
    elif op == 12:                                 # integer-cell 2-D convolve (i8 matrix cores), both modes: bit-identical
        choice = int(rng.integers(0, 4))
        if choice == 0:
            kernel = ["Disk:%.1f" % rng.uniform(2.0, 16.4), "Octagon:%d" % rng.integers(2, 16),
                      "Diamond:%d" % rng.integers(2, 16), "Plus:%d" % rng.integers(2, 16),
                      "Ring:%d,%d" % (rng.integers(2, 6), rng.integers(7, 16)),
                      "Rectangle:%dx%d" % (rng.integers(5, 66), rng.integers(2, 9))][int(rng.integers(0, 6))]
        else:
            kw, kh = int(rng.integers(5, 34)), int(rng.integers(5, 12))
            cells = rng.integers(0 if choice < 3 else -9, 10, (kh, kw)).astype(np.float64)
            cells[rng.random((kh, kw)) < 0.1] = np.nan
            if not (np.nansum(np.abs(cells)) > 0) or abs(np.nansum(cells)) < 1:
                cells[kh // 2, kw // 2] = 77.0
            kernel = "%dx%d+%d+%d: %s" % (kw, kh, rng.integers(0, kw), rng.integers(0, kh), " ".join(
                ",".join("nan" if np.isnan(v) else "%d" % v for v in r) for r in cells))
        layout = int(rng.integers(0, 3))               # RGBA alpha-weighted, four plain channels, RGB
        fast = rng.random() < 0.3
        if rng.random() < 0.3:
            # the same on a float-Quantum frame of integer samples (sometimes with one that is not:
            # the generic kernel behind the integer one then does the frame)
            fpx = px.astype(np.float32)
            if rng.random() < 0.25:
                fpx[int(rng.integers(0, rows)), int(rng.integers(0, cols)), int(rng.integers(0, 4))] = \
                    [0.5, -1.0, 65536.0, 12345.678][int(rng.integers(0, 4))]
            if layout == 2:
                fpx = np.ascontiguousarray(fpx[:, :, :3])
            if layout == 1:
                want = np.concatenate([refmod.RefImage(fpx[:, :, c].copy()).set_artifact("convolve:scale", "!")
                                       .morphology("Convolve", 1, kernel).numpy().reshape(rows, cols, 1) for c in range(4)], axis=2)
            else:
                want = refmod.RefImage(fpx).set_artifact("convolve:scale", "!").morphology("Convolve", 1, kernel).numpy()
            got = im.morphology_image(dev_float(fpx, has_alpha=layout == 0) if layout != 2 else dev_float(fpx),
                                      "Convolve", 1, kernel, scale=(1.0, 1)).numpy()
            failures += check_bits("integer convolve 2-D, float frame", got, want, detail + " layout %d %s" % (layout, kernel[:60]))
            return failures
        if layout == 0:
            image, want = dev(px), ref.set_artifact("convolve:scale", "!").morphology("Convolve", 1, kernel).numpy()
        elif layout == 1:
            image = dev(px, has_alpha=False)
            want = np.concatenate([refmod.RefImage(px[:, :, c].copy()).set_artifact("convolve:scale", "!")
                                   .morphology("Convolve", 1, kernel).numpy().reshape(rows, cols, 1) for c in range(4)], axis=2)
        else:
            rgb = np.ascontiguousarray(px[:, :, :3])
            image = dev(rgb)
            want = refmod.RefImage(rgb).set_artifact("convolve:scale", "!").morphology("Convolve", 1, kernel).numpy()
        if fast:
            im.set_precision(im.PRECISION_FAST)
        got = im.morphology_image(image, "Convolve", 1, kernel, scale=(1.0, 1)).numpy()
        im.set_precision(im.PRECISION_EXACT)
        failures += check("integer convolve 2-D", got, want, 1 if fast else 0, detail + " layout %d %s %s" % (
            layout, "fast" if fast else "exact", kernel[:60]))
    elif op == 13:                                 # any-cell 2-D convolve (fused fp64 + tie check): bit-identical
        kw, kh = int(rng.integers(3, 24)), int(rng.integers(3, 16))
        if kw * kh < 25:
            kw, kh = 7, 5
        signed_cells = rng.random() < 0.3
        cells = rng.uniform(-1.0 if signed_cells else 0.0, 1.0, (kh, kw))
        cells[rng.random((kh, kw)) < 0.1] = np.nan
        cells[kh // 2, kw // 2] = 3.0
        kernel = "%dx%d+%d+%d: %s" % (kw, kh, rng.integers(0, kw), rng.integers(0, kh), " ".join(
            ",".join("nan" if np.isnan(v) else "%.17g" % v for v in r) for r in cells))
        channels = int(rng.integers(1, 5))
        blend = channels in (2, 4) and rng.random() < 0.6
        is_float = rng.random() < 0.5
        frame = float_pixels(rows, cols, kind) if is_float else px
        if channels < 4:
            frame = np.ascontiguousarray(frame[:, :, 4 - channels:] if blend else frame[:, :, :channels])
        if blend or channels in (1, 3):
            want = refmod.RefImage(frame).set_artifact("convolve:scale", "!").morphology("Convolve", 1, kernel).numpy()
        else:
            want = np.concatenate([refmod.RefImage(frame[:, :, c].copy()).set_artifact("convolve:scale", "!")
                                   .morphology("Convolve", 1, kernel).numpy().reshape(rows, cols, 1) for c in range(channels)], axis=2)
        image = (dev_float if is_float else dev)(frame, has_alpha=blend)
        got = im.morphology_image(image, "Convolve", 1, kernel, scale=(1.0, 1)).numpy()
        what = detail + " c%d blend=%s %s" % (channels, blend, kernel[:50])
        failures += check_bits("fused 2-D convolve, float", got, want, what) if is_float else \
            check("fused 2-D convolve", got, want, 0, what)
    elif op == 14:                                 # ResizeImage
        filt = ["Lanczos", "Mitchell", "Catrom", "Triangle", "Hermite", "Gaussian", "Spline", "Lanczos2", "Cubic",
                "Box", "Point", "Hann", "Robidoux"][int(rng.integers(0, 13))]
        rows2, cols2 = int(rng.integers(1, 150)), int(rng.integers(1, 200))
        shape = int(rng.integers(0, 4))
        if shape == 0:                             # whole-number horizontal factor, the vertical one at least as large
            f = int(rng.integers(2, 5))
            target = (f * cols2, int(rng.integers(f * rows2, 5 * rows2 + 2)))
        elif shape == 1:                           # any enlargement
            target = (int(rng.integers(cols2, 4 * cols2 + 2)), int(rng.integers(rows2, 4 * rows2 + 2)))
        elif shape == 2:                           # reduction
            target = (int(rng.integers(1, cols2 + 1)), int(rng.integers(1, rows2 + 1)))
        else:                                      # mixed
            target = (int(rng.integers(1, 3 * cols2 + 2)), int(rng.integers(1, 3 * rows2 + 2)))
        is_float = rng.random() < 0.4
        alpha = rng.random() < 0.6
        fast = rng.random() < 0.6
        frame = float_pixels(rows2, cols2, int(rng.integers(0, 6))) if is_float else pixels(rows2, cols2, kind)
        if alpha:
            want = refmod.RefImage(frame).resize(target[0], target[1], filt).numpy()
        else:
            want = np.concatenate([refmod.RefImage(frame[:, :, c].copy()).resize(target[0], target[1], filt).numpy()
                                   .reshape(target[1], target[0], 1) for c in range(4)], axis=2)
        image = (dev_float if is_float else dev)(frame, has_alpha=alpha)
        if fast:
            im.set_precision(im.PRECISION_FAST)
        got = im.resize_image(image, target[0], target[1], filt).numpy()
        im.set_precision(im.PRECISION_EXACT)
        what = "%dx%d -> %dx%d %s %s %s kind %d" % (cols2, rows2, target[0], target[1], filt,
                                                      "alpha" if alpha else "plain", "fast" if fast else "exact", kind)
        if is_float:
            scale = float(np.nanmax(np.abs(np.where(np.isfinite(frame), frame, 0.0)))) if frame.size else 0.0
            failures += check_ulp("float resize", got, want, 1, what, residue=1.0e-9 * scale) if fast else \
                check_bits("float resize", got, want, what)
        else:
            failures += check("resize", got, want, 1 if fast else 0, what)
    elif op == 15:                                 # FAST blur family on every layout
        channels = int(rng.integers(1, 5))
        blend = channels in (2, 4) and rng.random() < 0.6
        frame = np.ascontiguousarray(px[:, :, 4 - channels:] if blend else px[:, :, :channels])
        which = int(rng.integers(0, 3))
        sigma = float(rng.uniform(0.3, 13.4)) if which != 1 else float(rng.uniform(0.8, 4.5))
        gain, threshold = float(rng.uniform(0.3, 3.0)), float(rng.uniform(0.0, 0.2))
        radius = blur_radius(sigma) if which != 1 else 0.0

        def reference(a):
            r = refmod.RefImage(a)
            return (r.blur(radius, sigma) if which == 0 else r.gaussian_blur(0.0, sigma) if which == 1 else
                    r.unsharp(radius, sigma, gain, threshold)).numpy()
        if blend or channels in (1, 3):
            want = reference(frame).reshape(rows, cols, channels)
        else:
            want = np.concatenate([reference(frame[:, :, c].copy()).reshape(rows, cols, 1) for c in range(channels)], axis=2)
        image = dev(frame, has_alpha=blend)
        im.set_precision(im.PRECISION_FAST)
        got = (im.blur_image(image, radius, sigma) if which == 0 else im.gaussian_blur_image(image, 0.0, sigma) if which == 1 else
               im.unsharp_mask_image(image, radius, sigma, gain, threshold)).numpy().reshape(rows, cols, channels)
        im.set_precision(im.PRECISION_EXACT)
        what = detail + " %s c%d blend=%s %gx%.3f" % (("blur", "gaussian", "unsharp")[which], channels, blend, radius, sigma)
        if which == 2:
            blurred = (refmod.RefImage(frame).blur(radius, sigma).numpy().reshape(rows, cols, channels).astype(np.int64)
                       if (blend or channels in (1, 3)) else None)
            d = np.abs(got.astype(np.int64) - want.astype(np.int64))
            if blurred is not None:
                edge = np.abs(2 * np.abs(frame.astype(np.int64) - blurred) - 65535.0 * threshold) <= 2.0
                d[edge] = 0
                failures += check("fast unsharp, layout", d, np.zeros_like(d), int(np.ceil(1.0 + gain)), what)
        else:
            failures += check("fast blur, layout", got, want, 1, what)
    else:                                          # FAST Lab
        im.set_precision(im.PRECISION_FAST)
        d2 = dev(px)
        im.transform_image_colorspace(d2, "Lab")
        im.set_precision(im.PRECISION_EXACT)
        failures += check("fast lab", d2.numpy(), ref.colorspace("Lab").numpy(), 1, detail)
    return failures


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    setup(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    only_ops = [int(t) for t in os.environ.get("STRESS_OPS", "").split(",") if t.strip()]
    t0 = time.time()
    cases = failures = 0
    while time.time() - t0 < budget:
        failures += run_case(only_ops[int(rng.integers(0, len(only_ops)))] if only_ops else None)
        cases += 1
    print("%d cases, %d failures, %.0f s" % (cases, failures, time.time() - t0))
    sys.exit(1 if failures else 0)


if __name__ == "__main__":
    main()
