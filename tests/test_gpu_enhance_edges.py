"""Edge shapes, channel masks, alpha structure, float specials and both precisions for the nine enhance / effect
operators that had one small random frame each: MotionBlurImage, RotationalBlurImage, LocalContrastImage,
DespeckleImage, WaveletDenoiseImage (effects.hip: one thread per column, 256-thread blocks) and ContrastImage,
ModulateImage, FunctionImage, GrayscaleImage (pointwise.hip: grid-stride loops under stream_grid's block cap).

Every case goes through the C ABI and is compared with the compiled reference (oracle/_ref) on the same input.
Bars (the project's contract, nothing new): bit-identical for Q16 and float Quantum; where the device's sin / asin /
atan is involved (ContrastImage, FunctionImage Sinusoid / Arcsin / Arctan) Q16 within one level and float within
one ULP, as test_function and test_contrast_and_modulate; ModulateImage at percentages that are multiples of ten: at
most one level on fewer than 0.5 % of the samples (test_modulate_colour_models); NaN positions equal and the rest
bit for bit (test_local_contrast)."""
import ctypes

import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32

# The sizes of the grid-stride cases follow three constants of layout_dispatch.hpp and pointwise.hip (stream_grid's block cap, the block
# width and kPointBatch); tests/test_enhance_edge_sizes.py reads them from the source and fails when these frames
# stop being "just above" one trip of the loops.
STREAM_CAP_BLOCKS, BLOCK_WIDTH, POINT_BATCH = 8192, 256, 4
BIG_STREAM_SHAPE = (1449, 1449)           # 2 099 601 pixels: 0.12 % above 8192*256 (function_kernel, grayscale_kernel)
BIG_TONE_SHAPE = (2897, 2897)             # 8 392 609 pixels: 0.05 % above 8192*256*4, odd (tone_kernel's ragged batch)
GUARD_ROWS = 2                            # sentinel rows behind a big frame: more than the 768 pixels a batch can overrun

# one thread per column in 256-thread blocks: widths on both sides of one and two blocks; 254 and 255 put
# despeckle_load_kernel's padded width W+2 there, 86 and 257 put wavelet_hat_kernel's W*colour there (colour 3 and 1)
BOUNDARY_WIDTHS = [86, 254, 255, 256, 257, 300, 513]
BOUNDARY_ROWS = 36                        # WaveletDenoiseImage needs 33

DEGENERATE_SHAPES = [(1, 1), (1, 40), (40, 1), (2, 2), (2, 300), (300, 2)]

MORPH_OPS = {                             # name: (binding function, RefImage method, arguments)
    "motion": ("motion_blur_image", "motion_blur", (0.0, 3.0, 30.0)),
    "rotational": ("rotational_blur_image", "rotational_blur", (12.0,)),
    "local_contrast": ("local_contrast_image", "local_contrast", (60.0, 40.0)),
    "despeckle": ("despeckle_image", "despeckle", ()),
    "wavelet": ("wavelet_denoise_image", "wavelet_denoise", (5000.0, 0.4)),
}
C_NAMES = {"motion": "MagickHipMotionBlurImage", "rotational": "MagickHipRotationalBlurImage",
           "local_contrast": "MagickHipLocalContrastImage", "despeckle": "MagickHipDespeckleImage",
           "wavelet": "MagickHipWaveletDenoiseImage"}

POINT_OPS = {                             # name: (binding function, RefImage method, arguments, libm involved)
    "function_polynomial": ("function_image", "function", ("Polynomial", (0.3, -1.2, 1.5, 0.1)), False),
    "function_sinusoid": ("function_image", "function", ("Sinusoid", (3.0, 90.0, 0.4, 0.5)), True),
    "contrast": ("contrast_image", "contrast", (True,), True),
    "modulate_hsl": ("modulate_image", "modulate", (113.0, 87.0, 131.0), False),
    "modulate_hsb": ("modulate_image", "modulate", (113.0, 87.0, 131.0, "HSB"), False),
    "grayscale_rec709luma": ("grayscale_image", "grayscale", ("Rec709Luma",), False),
    "grayscale_average": ("grayscale_image", "grayscale", ("Average",), False),
}


def check(got, want, what, libm=False):
    """The bar of the module docstring; NaN positions equal, everything else by assert_parity."""
    got = got.reshape(want.shape)
    if want.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ (%d vs %d)" % (
            what, int(np.isnan(got).sum()), int(nan.sum()))
        got, want = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
        assert_parity(got, want, True, what, max_ulp=1 if libm else 0)
    else:
        assert_parity(got, want, not libm, what)


def local_contrast_width(rows, cols, radius):
    """effect.c:2067-2068: the blur width comes from the longer side."""
    return int(max(rows, cols) * 0.002 * abs(radius))


def declines(name, rows, cols, args):
    """The decline conditions stated in effects.hip (launch_wavelet_denoise, launch_local_contrast)."""
    if name == "wavelet":
        return rows < 33 or cols < 33
    if name == "local_contrast":
        w = local_contrast_width(rows, cols, args[0])
        return w < 1 or cols <= 2 * w + 2
    return False


def run_morph(im, refmod, name, px, args=None, mask=None, copy=(), host=False, what=""):
    """One of the five effects.hip operators on `px` against the reference; a frame the library is documented to
    decline must raise, any other must match."""
    fn, method, default = MORPH_OPS[name]
    args = default if args is None else args
    rows, cols = px.shape[:2]
    image = im.Image(px.copy() if host else to_device(px), copy_channels=copy)
    what = "%s %s %s %dx%dx%d %s" % (name, args, px.dtype.name, rows, cols, px.shape[2], what)
    if declines(name, rows, cols, args):
        with pytest.raises(im.MagickHipError):
            getattr(im, fn)(image, *args)
        return None
    got = getattr(im, fn)(image, *args).numpy()
    ref = refmod.RefImage(px)
    if mask is not None:
        ref.set_channel_mask(mask)
    check(got, getattr(ref, method)(*args).numpy(), what)
    return got


def run_point(im, refmod, name, px, colorspace="sRGB", mask=None, copy=(), what="", args=None):
    fn, method, default, libm = POINT_OPS[name]
    args = default if args is None else args
    image = im.Image(to_device(px), colorspace=colorspace, copy_channels=copy)
    getattr(im, fn)(image, *args)
    got = image.numpy()
    ref = refmod.RefImage(px, colorspace)
    if mask is not None:
        ref.set_channel_mask(mask)
    want = getattr(ref, method)(*args).numpy()
    compare_point(name, got, want, px, "%s %s %s %s %s" % (name, args, px.dtype.name, px.shape, what), libm)
    return got


def compare_point(name, got, want, px, what, libm):
    if name.startswith("grayscale"):       # the reference re-lays the frame out as gray[+alpha] (SetImageColorspace)
        check(np.ascontiguousarray(got[:, :, 0]), np.ascontiguousarray(want[:, :, 0]), what, libm)
        if px.shape[2] in (2, 4):
            check(np.ascontiguousarray(got[:, :, -1]), np.ascontiguousarray(want[:, :, -1]), what + " alpha")
        for c in range(1, px.shape[2] - (1 if px.shape[2] in (2, 4) else 0)):   # SetPixelGray: the first channel only
            check(np.ascontiguousarray(got[:, :, c]), np.ascontiguousarray(px[:, :, c]), what + " channel %d kept" % c)
    else:
        check(got, want, what, libm)


def ramp_frame(rows, cols, channels, dtype, guard_rows=0):
    """Channel c of pixel i is (i*(3+2c) + 9973c) mod 65521 (+0.25 on float frames): 65521 is prime and no power of
    two, so a pixel differs in every channel from the one 8192*256 or 8192*256*4 positions before it — a pixel a
    grid-stride loop skips or visits twice shows.  guard_rows more rows of the level 4242 follow the frame."""
    i = np.arange((rows + guard_rows) * cols, dtype=np.int64)
    px = np.empty((rows + guard_rows, cols, channels), dtype=dtype)
    for c in range(channels):
        level = ((i * (3 + 2 * c) + 9973 * c) % 65521).reshape(rows + guard_rows, cols)
        px[:, :, c] = level.astype(dtype) + (dtype(0.25) if dtype == HDRI else dtype(0))
    px[rows:] = 4242
    return px


def alpha_frames(rows, cols, channels, dtype):
    """The alpha structures that broke the blur kernels (adversarial_blur_frames): binary alpha, 0..3-level alpha, a
    sprite on transparent ground, and a fully transparent frame (gamma == 0: PerceptibleReciprocal clamps)."""
    rng = np.random.default_rng(47)
    base = rng.integers(0, 65536, (rows, cols, channels), dtype=np.uint16)
    binary, tiny, sprite, clear = base.copy(), base.copy(), base.copy(), base.copy()
    binary[:, :, -1] = np.where(rng.random((rows, cols)) < 0.5, 0, 65535)
    tiny[:, :, -1] = rng.integers(0, 4, (rows, cols), dtype=np.uint16)
    sprite[:, :, -1] = 0
    for _ in range(5):
        y0, x0 = int(rng.integers(0, max(1, rows - 2))), int(rng.integers(0, max(1, cols - 2)))
        sprite[y0: y0 + int(rng.integers(1, 20)), x0: x0 + int(rng.integers(1, 20)), -1] = 65535
    clear[:, :, -1] = 0
    frames = {"binary": binary, "tiny": tiny, "sprite": sprite, "transparent": clear}
    if dtype == HDRI:
        frames = {k: v.astype(np.float32) + (np.float32(0.375) if k != "transparent" else np.float32(0)) * (v > 0)
                  for k, v in frames.items()}
    return frames


# ------------------------------------------------------------------ block boundaries
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("cols", BOUNDARY_WIDTHS)
@pytest.mark.parametrize("name", list(MORPH_OPS))
def test_block_boundaries(im, refmod, name, cols, channels, dtype):
    """blockIdx.x > 0 and the ragged last block of the one-thread-per-column kernels."""
    px = make_pixels(BOUNDARY_ROWS, cols, channels, dtype, seed=cols + channels)
    run_morph(im, refmod, name, px)


# ------------------------------------------------------------------ grid-stride second trip
def big_frame_case(im, refmod, name, shape, channels, dtype, colorspace="sRGB"):
    rows, cols = shape
    full = ramp_frame(rows, cols, channels, dtype, GUARD_ROWS)
    px = full[:rows]
    tensor = to_device(full)
    fn, method, args, libm = POINT_OPS[name]
    image = im.Image(tensor[:rows], colorspace=colorspace)
    getattr(im, fn)(image, *args)
    got = image.numpy()
    guard = im.Image(tensor[rows:], has_alpha=False).numpy()
    assert (guard == 4242).all(), "%s wrote behind the frame's last pixel" % name
    want = getattr(refmod.RefImage(px, colorspace), method)(*args).numpy()
    compare_point(name, got, want, px, "%s %s on %dx%dx%d %s" % (name, args, rows, cols, channels, np.dtype(dtype).name), libm)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels,colorspace", [(4, "sRGB"), (3, "RGB")])
@pytest.mark.parametrize("name", ["function_polynomial", "function_sinusoid", "grayscale_rec709luma", "grayscale_average"])
def test_grid_stride_second_trip_one_pixel_per_thread(im, refmod, name, channels, colorspace, dtype):
    """function_kernel / grayscale_kernel: stream_grid caps the grid at 8192 blocks of 256, so the loop takes a second
    trip just above 2 097 152 pixels."""
    assert BIG_STREAM_SHAPE[0] * BIG_STREAM_SHAPE[1] > STREAM_CAP_BLOCKS * BLOCK_WIDTH
    big_frame_case(im, refmod, name, BIG_STREAM_SHAPE, channels, dtype, colorspace)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("name", ["contrast", "modulate_hsl", "modulate_hsb"])
def test_grid_stride_second_trip_four_pixels_per_thread(im, refmod, name, channels, dtype):
    """tone_kernel moves kPointBatch pixels per thread: a second trip just above 8 388 608 pixels; the count is no
    multiple of 256*kPointBatch, so the clamped tail loads and the guarded stores run in that trip."""
    n = BIG_TONE_SHAPE[0] * BIG_TONE_SHAPE[1]
    assert n > STREAM_CAP_BLOCKS * BLOCK_WIDTH * POINT_BATCH and n % (BLOCK_WIDTH * POINT_BATCH) != 0
    big_frame_case(im, refmod, name, BIG_TONE_SHAPE, channels, dtype)


# ------------------------------------------------------------------ degenerate shapes
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
@pytest.mark.parametrize("name", ["despeckle", "local_contrast", "wavelet"])
def test_degenerate_shapes(im, refmod, name, shape, channels, dtype):
    """LocalContrastImage takes (1,40) and (2,300) (w = 4 and 36 from the columns); it declines the others and
    WaveletDenoiseImage declines all of them: run_morph asserts the decline."""
    run_morph(im, refmod, name, make_pixels(shape[0], shape[1], channels, dtype, seed=5))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("angle", [30.0, 135.0, 210.0, -45.0])
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
def test_motion_blur_degenerate_shapes(im, refmod, shape, angle, channels, dtype):
    """sigma 3 gives offsets up to 8 pixels; the four angles send them off a 1-wide and a 1-tall frame on every side."""
    run_morph(im, refmod, "motion", make_pixels(shape[0], shape[1], channels, dtype, seed=6), args=(0.0, 3.0, angle))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("angle", [0.5, 90.0, 359.0])
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES + [(7, 8), (8, 7), (9, 9), (8, 8), (61, 64), (64, 61)])
def test_rotational_blur_shapes_and_angles(im, refmod, shape, angle, channels, dtype):
    """Even sizes put the centre on a half-integer, odd ones on a pixel (radius == 0 there: step stays 1).  0.5 degrees
    gives n = 2 samples, so step clamps to n-1 everywhere inside half the blur radius; 359 degrees gives the large
    counts; at 90 degrees on the 61- and 64-pixel frames the pixels next to the centre reach step >= n."""
    run_morph(im, refmod, "rotational", make_pixels(shape[0], shape[1], channels, dtype, seed=7), args=(angle,))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels,colorspace", [(4, "sRGB"), (3, "RGB")])
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
@pytest.mark.parametrize("name", list(POINT_OPS))
def test_pointwise_degenerate_shapes(im, refmod, name, shape, channels, colorspace, dtype):
    if not name.startswith("grayscale"):
        colorspace = "sRGB"
    run_point(im, refmod, name, make_pixels(shape[0], shape[1], channels, dtype, seed=8), colorspace=colorspace)


# ------------------------------------------------------------------ decline thresholds
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("shape", [(33, 33), (33, 257), (257, 33), (32, 40), (40, 32)])
def test_wavelet_denoise_threshold(im, refmod, shape, channels, dtype):
    """33 x 33 is the first size taken (two spans of the coarsest level); 32 in either direction is declined."""
    assert declines("wavelet", shape[0], shape[1], ()) == (min(shape) < 33)
    run_morph(im, refmod, "wavelet", make_pixels(shape[0], shape[1], channels, dtype, seed=9))


LOCAL_CONTRAST_THRESHOLDS = [
    # rows, cols, radius, w, accepted
    (9, 13, 200.0, 5, True),              # w from the columns: 13*0.002*200 = 5.2; 13 == 2w+3
    (9, 12, 220.0, 5, False),             #                      12*0.002*220 = 5.28; 12 == 2w+2
    (400, 19, 11.0, 8, True),             # w from the rows of a tall frame: 400*0.002*11 = 8.8; 19 == 2w+3
    (400, 18, 11.0, 8, False),            #                                                      18 == 2w+2
    (40, 500, 10.0, 10, True),            # 500*0.002*10 is 10 in exact arithmetic: the truncation agrees
    (30, 1000, 1.0, 2, True),             # 1000*0.002*1 likewise 2
    (30, 400, 1.0, 0, False),             # w == 0
]


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("rows,cols,radius,w,accepted", LOCAL_CONTRAST_THRESHOLDS)
def test_local_contrast_threshold(im, refmod, rows, cols, radius, w, accepted, channels, dtype):
    assert local_contrast_width(rows, cols, radius) == w
    assert declines("local_contrast", rows, cols, (radius, 40.0)) == (not accepted)
    run_morph(im, refmod, "local_contrast", make_pixels(rows, cols, channels, dtype, seed=10), args=(radius, 40.0))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("name,shape,args", [("wavelet", (32, 40), (5000.0, 0.4)), ("wavelet", (40, 32), (5000.0, 0.4)),
                                             ("local_contrast", (9, 12), (220.0, 40.0)),
                                             ("local_contrast", (400, 18), (11.0, 40.0))])
def test_declined_call_leaves_the_output_alone(im, name, shape, args, dtype):
    from imagemagick_amd import _lib
    px = make_pixels(shape[0], shape[1], 4, dtype, seed=11)
    filled = make_pixels(shape[0], shape[1], 4, dtype, seed=12)
    for host in (False, True):
        image = im.Image(px.copy() if host else to_device(px))
        out = im.Image(filled.copy() if host else to_device(filled))
        with pytest.raises(im.MagickHipError):
            _lib.check(getattr(_lib.load(), C_NAMES[name])(ctypes.byref(image.descriptor()),
                                                         ctypes.byref(out.descriptor()), *args))
        assert out.numpy().tobytes() == filled.tobytes(), "%s %s: a declined call wrote to its output" % (name, shape)
        assert image.numpy().tobytes() == px.tobytes()


# ------------------------------------------------------------------ channel masks
MASKS = [("RG", (2, 3)), ("RGB", (3,)), ("A", (0, 1, 2))]


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask,copy", MASKS)
@pytest.mark.parametrize("name", list(MORPH_OPS))
def test_channel_mask_rgba(im, refmod, name, mask, copy, dtype):
    """Each kernel has its own rule: motion and rotational blur copy the centre pixel, despeckle the original,
    LocalContrastImage looks at the traits of R, G, B only, WaveletDenoiseImage rebuilds every colour channel whatever
    its traits (visual-effects.c:3590-3598)."""
    px = make_pixels(45, 70, 4, dtype, seed=13)
    got = run_morph(im, refmod, name, px, mask=mask, copy=copy, what="-channel " + mask)
    if name != "wavelet":
        for c in copy:
            assert np.array_equal(got[:, :, c], px[:, :, c]), "%s -channel %s changed channel %d" % (name, mask, c)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("name", list(MORPH_OPS))
def test_channel_mask_gray_alpha(im, refmod, name, dtype):
    px = make_pixels(45, 70, 2, dtype, seed=14)
    got = run_morph(im, refmod, name, px, mask="R", copy=(1,), what="-channel Gray")
    assert np.array_equal(got[:, :, 1], px[:, :, 1])


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask,copy", MASKS)
@pytest.mark.parametrize("name", list(POINT_OPS))
def test_channel_mask_pointwise(im, refmod, name, mask, copy, dtype):
    """FunctionImage skips the channels outside the mask (statistic.c:1133-1137).  ContrastImage, ModulateImage and
    GrayscaleImage write R, G, B (Gray) whatever the mask says (enhance.c: SetPixelRed / Green / Blue / Gray without a
    look at the traits) and so does the library: the comparison with the masked reference pins that."""
    px = make_pixels(41, 57, 4, dtype, seed=15)
    got = run_point(im, refmod, name, px, mask=mask, copy=copy, what="-channel " + mask)
    if name.startswith("function"):
        for c in copy:
            assert np.array_equal(got[:, :, c], px[:, :, c]), "%s -channel %s changed channel %d" % (name, mask, c)


# ------------------------------------------------------------------ alpha structure
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [4, 2])
@pytest.mark.parametrize("kind", ["binary", "tiny", "sprite", "transparent"])
@pytest.mark.parametrize("name,args", [("motion", (0.0, 3.0, 30.0)), ("motion", (0.0, 6.0, -110.0)),
                                       ("rotational", (12.0,)), ("rotational", (200.0,))])
def test_alpha_structure(im, refmod, name, args, kind, channels, dtype):
    """gray + alpha is motion_blur_kernel<Q,2,true>, which no other test instantiates."""
    run_morph(im, refmod, name, alpha_frames(50, 66, channels, dtype)[kind], args=args, what=kind + " alpha")


# ------------------------------------------------------------------ float specials
def special_frame(kind, channels=4, rows=48, cols=64):
    rng = np.random.default_rng(53)
    px = (rng.random((rows, cols, channels)) * 65535.0).astype(np.float32)
    if kind == "negative":
        px[10:20, 12:30, :] = -(rng.random((10, 18, channels)) * 30000.0).astype(np.float32)
    elif kind == "above":
        px[10:20, 12:30, :] = (65535.0 + rng.random((10, 18, channels)) * 90000.0).astype(np.float32)
    elif kind == "inf":
        px[12, 14, 0], px[30, 40, 1] = np.inf, -np.inf
        px[20, 50, channels - 1] = np.inf
    elif kind == "nan":
        px[22:25, 30:34, :] = np.nan
    elif kind == "subnormal":
        px[10:20, 12:30, :] = (rng.random((10, 18, channels)) * 1.0e-39).astype(np.float32)
    elif kind == "zeros":                  # zero luma for LocalContrastImage, zero saturation for Contrast / Modulate
        px[10:20, 12:30, :] = 0.0
        px[30:40, 12:30, :max(1, channels - 1)] = px[30:40, 12:30, :1]
    elif kind == "hull":                   # Hull's >= guard: neighbours exactly 514 and just under 514 apart
        px[:, :, :] = 1000.0
        px[8:40:4, 8:56:4, :] = 1514.0
        px[10:40:4, 10:56:4, :] = np.float32(1513.99997)
        px[9:40:4, 9:56:4, :] = 486.0
        px[11:40:4, 11:56:4, :] = np.float32(486.00003)
    else:
        raise ValueError(kind)
    return px


SPECIALS = ["negative", "above", "inf", "nan", "subnormal", "zeros"]


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("name,kind", [(n, k) for n in MORPH_OPS for k in SPECIALS] + [("despeckle", "hull")])
def test_float_specials(im, refmod, name, kind, channels):
    run_morph(im, refmod, name, special_frame(kind, channels), what=kind)


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("kind", SPECIALS)
@pytest.mark.parametrize("name", list(POINT_OPS))
def test_float_specials_pointwise(im, refmod, name, kind, channels):
    run_point(im, refmod, name, special_frame(kind, channels), what=kind)


# ------------------------------------------------------------------ Q16 rounding ties
def test_function_polynomial_on_rounding_ties(im, refmod):
    """0.5*x + 0 on odd levels: every result is x.5 before rounding."""
    px = make_pixels(64, 80, 4, Q16, seed=16) | np.uint16(1)
    run_point(im, refmod, "function_polynomial", px, args=("Polynomial", (0.5, 0.0)), what="ties")
    run_point(im, refmod, "function_polynomial", px, args=("Polynomial", (0.25, 0.25, 0.0)), what="ties")
    run_point(im, refmod, "function_polynomial", px.astype(np.float32), args=("Polynomial", (0.5, 0.0)), what="ties")


@pytest.mark.parametrize("method", ["Average", "Lightness", "Brightness", "Rec709Luma"])
@pytest.mark.parametrize("channels,colorspace", [(4, "sRGB"), (3, "RGB")])
def test_grayscale_on_rounding_ties(im, refmod, method, channels, colorspace):
    """Q16: sums of every residue mod 3 (Average) and odd min+max (Lightness: x.5).  Float: half-integer samples
    whose sum is 1.5 mod 3 (Average on x.5) on top."""
    rng = np.random.default_rng(17)
    px = make_pixels(60, 90, channels, Q16, seed=17)
    px[:, :, 1] = px[:, :, 0] + (np.arange(90) % 3)[None, :].astype(np.uint16)        # r+g+b = 3r + 0 / 1 / 2 + ...
    px[:, :, 2] = px[:, :, 0] + np.uint16(1)
    px[:, 45:, 2] = px[:, 45:, 0] ^ np.uint16(1)                                      # min+max odd
    run_point(im, refmod, "grayscale_average", px, colorspace=colorspace, args=(method,), what="ties")
    fpx = px.astype(np.float32)
    fpx[:, :, 0] += np.float32(0.5)
    fpx[:, ::2, 1] += np.float32(0.5)
    fpx[:, 1::2, 2] += np.float32(0.5) * rng.integers(0, 2, (60, 45)).astype(np.float32)
    run_point(im, refmod, "grayscale_average", fpx, colorspace=colorspace, args=(method,), what="float ties")


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("angle,sigma", [(0.0, 2.0), (90.0, 2.0), (180.0, 5.0), (45.0, 3.0)])
def test_motion_blur_on_alternating_levels(im, refmod, angle, sigma, channels):
    """v, v+1, v, ... along the motion direction: the sums sit next to x.5 wherever the taps of either parity add up
    to a half."""
    rows, cols = 40, 70
    y, x = np.mgrid[0:rows, 0:cols]
    along = x if angle in (0.0, 180.0) else y if angle == 90.0 else x + y
    px = np.empty((rows, cols, channels), dtype=np.uint16)
    for c, level in enumerate((1000, 32767, 65533, 40000)[:channels]):
        px[:, :, c] = level + (along & 1)
    if channels in (2, 4):
        px[:, :, -1] = 65534 + ((x + y) & 1)
    run_morph(im, refmod, "motion", px, args=(0.0, sigma, angle), what="alternating levels")
    run_morph(im, refmod, "motion", px.astype(np.float32), args=(0.0, sigma, angle), what="alternating levels")


# ------------------------------------------------------------------ both precisions
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("name", list(MORPH_OPS) + list(POINT_OPS))
def test_fast_and_exact_return_the_same_bits(im, refmod, name, dtype):
    """The suite runs in EXACT; the library's default is FAST.  None of the nine operators takes a precision: both
    modes must give the same bits, and those must meet the operator's EXACT bar."""
    px = make_pixels(120, 160, 4, dtype, seed=18)
    results = {}
    try:
        for precision in (im.PRECISION_FAST, im.PRECISION_EXACT):
            im.set_precision(precision)
            if name in MORPH_OPS:
                results[precision] = run_morph(im, refmod, name, px, what="precision %d" % precision)
            else:
                results[precision] = run_point(im, refmod, name, px, what="precision %d" % precision)
    finally:
        im.set_precision(im.PRECISION_EXACT)
    assert results[im.PRECISION_FAST].tobytes() == results[im.PRECISION_EXACT].tobytes(), name + ": FAST != EXACT"
    # ... and the precision carried by the image (MhImage::precision) changes nothing either
    fn = MORPH_OPS[name][0] if name in MORPH_OPS else POINT_OPS[name][0]
    args = MORPH_OPS[name][2] if name in MORPH_OPS else POINT_OPS[name][2]
    image = im.Image(to_device(px), precision=im.PRECISION_FAST)
    out = getattr(im, fn)(image, *args)
    assert out.numpy().tobytes() == results[im.PRECISION_EXACT].tobytes(), name + ": per-image FAST != EXACT"


# ------------------------------------------------------------------ host-memory path
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("name", list(MORPH_OPS))
def test_host_memory_path(im, refmod, name, dtype):
    """MH_MEMORY_HOST: the library stages the pixel-cache block itself (as test_blur_host_memory_path)."""
    run_morph(im, refmod, name, make_pixels(57, 300, 4, dtype, seed=19), host=True, what="host memory")
