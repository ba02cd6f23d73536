"""The NumPy restatement of the level operators (tests/levels_oracle.py) and the library's host table
MhGammaLUT against the compiled reference, bit for bit, on both Quantum types.  No GPU."""
import numpy as np
import pytest

from statistic_oracle import assert_same
from levels_oracle import (CHANNELS, LAYOUTS, LEVELS, SIGMOIDALS, GAMMAS, ref_image, ref_level, ref_levelize, ref_gamma,
                           ref_negate, ref_sigmoidal, ref_min_max_stretch, ref_auto_level, ref_linear_stretch,
                           ref_normalize, ref_brightness_contrast, ref_range, linear_stretch_property, ramp, frame,
                           gray_pixels, seed_frame, constant, out_of_range_float, kept_channels_equal, level, levelize, gamma, gamma_map,
                           negate, sigmoidal, image_range, min_max_stretch, linear_stretch,
                           brightness_contrast_coefficients, polynomial)

Q16, HDRI = np.uint16, np.float32
# the stored offsets an RGBA frame writes under each mask
RGBA_MASKS = [("R", (0,)), ("RGB", (0, 1, 2)), ("A", (3,))]


@pytest.fixture(scope="module")
def lib():
    import imagemagick_amd
    imagemagick_amd.load()
    return imagemagick_amd


def inputs(layout, dtype):
    yield "ramp", ramp(CHANNELS[layout], dtype)
    yield "noise", frame(layout, 23, 31, dtype)
    if dtype == HDRI:
        yield "out of range", out_of_range_float(23, 31, CHANNELS[layout])


def every(px):
    return tuple(range(px.shape[2]))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_level_and_levelize_restatement(refmod, layout, dtype):
    for what, px in inputs(layout, dtype):
        for black, white, value in LEVELS:
            want = ref_level(ref_image(refmod, px), black, white, value).numpy()
            assert_same(level(px, every(px), black, white, value), want, "level %s %s %s" % (layout, what, (black, white, value)))
            want = ref_levelize(ref_image(refmod, px), black, white, value).numpy()
            assert_same(levelize(px, every(px), black, white, value), want,
                        "levelize %s %s %s" % (layout, what, (black, white, value)))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gamma_restatement(refmod, layout, dtype):
    for what, px in inputs(layout, dtype):
        for value in GAMMAS:
            want = ref_gamma(ref_image(refmod, px), value).numpy()
            assert_same(gamma(px, every(px), value), want, "gamma %s %s %g" % (layout, what, value))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_negate_restatement(refmod, layout, dtype):
    for what, px in inputs(layout, dtype):
        if CHANNELS[layout] >= 3:
            px = gray_pixels(px)
        for grayscale in (False, True):
            want = ref_negate(ref_image(refmod, px), grayscale).numpy()
            assert_same(negate(px, every(px), grayscale), want, "negate %s %s grayscale=%s" % (layout, what, grayscale))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sigmoidal_restatement(refmod, layout, dtype):
    for what, px in inputs(layout, dtype):
        for sharpen, contrast, midpoint in SIGMOIDALS:
            want = ref_sigmoidal(ref_image(refmod, px), sharpen, contrast, midpoint).numpy()
            assert_same(sigmoidal(px, every(px), sharpen, contrast, midpoint), want,
                        "sigmoidal %s %s %s" % (layout, what, (sharpen, contrast, midpoint)))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask,update", RGBA_MASKS)
def test_channel_masks(refmod, mask, update, dtype):
    """Only the channels of the mask are written, the others keep their bits; NegateImage reads
    IsPixelGray whatever the mask is."""
    px = gray_pixels(frame("rgba", 23, 31, dtype, seed=3))

    def image():
        return ref_image(refmod, px, mask=mask)

    assert_same(level(px, update, 5000.0, 60000.0, 2.2), ref_level(image(), 5000.0, 60000.0, 2.2).numpy(), "level " + mask)
    assert_same(levelize(px, update, 5000.0, 60000.0, 0.45), ref_levelize(image(), 5000.0, 60000.0, 0.45).numpy(),
                "levelize " + mask)
    assert_same(gamma(px, update, 2.2), ref_gamma(image(), 2.2).numpy(), "gamma " + mask)
    assert_same(negate(px, update, False), ref_negate(image(), False).numpy(), "negate " + mask)
    assert_same(negate(px, update, True), ref_negate(image(), True).numpy(), "negate gray " + mask)
    assert_same(sigmoidal(px, update, 1, 5.0, 32767.5), ref_sigmoidal(image(), 1, 5.0, 32767.5).numpy(), "sigmoidal " + mask)
    assert_same(sigmoidal(px, update, 0, 5.0, 32767.5), ref_sigmoidal(image(), 0, 5.0, 32767.5).numpy(),
                "inverse sigmoidal " + mask)
    assert image_range(px, update) == ref_range(image()), "range " + mask


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_range_and_min_max_stretch_restatement(refmod, layout, dtype):
    frames = [("noise", frame(layout, 23, 31, dtype)), ("narrow", (frame(layout, 23, 31, Q16) // 3 + 9000).astype(dtype))]
    if dtype == HDRI:
        frames.append(("out of range", out_of_range_float(23, 31, CHANNELS[layout])))
    for what, px in frames:
        assert image_range(px, every(px)) == ref_range(ref_image(refmod, px)), "range %s %s" % (layout, what)
        for black, white, value in ((0.0, 0.0, 1.0), (500.0, 1200.5, 1.0), (0.0, 0.0, 2.2), (300.0, 0.0, 0.45)):
            want = ref_min_max_stretch(ref_image(refmod, px), black, white, value).numpy()
            got = min_max_stretch(px, every(px), True, black, white, value)
            assert_same(got, want, "min-max %s %s %s" % (layout, what, (black, white, value)))
        assert_same(min_max_stretch(px, every(px), True, 0.0, 0.0, 1.0), ref_auto_level(ref_image(refmod, px)).numpy(),
                    "auto-level %s %s" % (layout, what))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_min_max_stretch_constant_frame_is_untouched(refmod, layout, dtype):
    px = constant(23, 31, CHANNELS[layout], dtype)
    want = ref_auto_level(ref_image(refmod, px)).numpy()
    assert_same(want, px, "the reference on a constant %s frame" % layout)
    assert_same(min_max_stretch(px, every(px), True, 0.0, 0.0, 1.0), want, "auto-level constant %s" % layout)
    # an all-zero frame: *maxima stays at MagickMinimumValue, below MagickEpsilon of the minimum
    zero = np.zeros_like(px)
    assert image_range(zero, every(zero)) == ref_range(ref_image(refmod, zero))
    assert_same(min_max_stretch(zero, every(zero), True, 0.0, 0.0, 1.0), ref_auto_level(ref_image(refmod, zero)).numpy(),
                "auto-level zero %s" % layout)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_range_is_seeded_with_column_0_of_channel_0(refmod, dtype):
    """GetImageRange starts every row from p[0], whatever the mask: the range of mask A of an RGBA
    frame covers alpha and column 0 of red."""
    px = (frame("rgba", 23, 31, Q16, seed=5) // 4 + 20000).astype(dtype)
    px[7, 0, 0] = 150
    px[11, 0, 0] = 64000
    px[3, 5, 0] = 10            # channel 0 outside column 0: not part of the range
    minimum, maximum = ref_range(ref_image(refmod, px, mask="A"))
    assert (minimum, maximum) == (150.0, 64000.0)
    assert image_range(px, (3,)) == (minimum, maximum)
    want = ref_auto_level(ref_image(refmod, px, mask="A")).numpy()
    # per-channel mode: the one Update channel is alpha, which is never levelled (see below)
    assert_same(min_max_stretch(px, (3,), False, 0.0, 0.0, 1.0), want, "auto-level mask A")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_per_channel_ranges_see_the_levelled_column_0(refmod, dtype):
    """In per-channel mode channel 0 is levelled before channel 1 is measured: with channel 0's
    extremes in column 0 the later ranges become 0 ... QuantumRange and channels 1 and 2 keep their bits."""
    px = seed_frame(dtype)
    want = ref_auto_level(ref_image(refmod, px, mask="RGB")).numpy()
    assert want[..., 0].min() == 0 and want[..., 0].max() == 65535
    assert kept_channels_equal(want, px, [1, 2])
    assert_same(min_max_stretch(px, (0, 1, 2), False, 0.0, 0.0, 1.0), want, "auto-level mask RGB")
    # one range for all the channels up front would level channels 1 and 2
    minimum, maximum = image_range(px, (1,))
    assert not np.array_equal(level(px, (1,), minimum, maximum, 1.0), px)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_per_channel_mask_is_a_channel_type_bit(refmod, dtype):
    """1 << offset is a ChannelType bit: offset 3 of RGBA selects Black, offset 1 of gray+alpha
    Green, so alpha is never levelled per channel; under the default mask it is."""
    px = (frame("rgba", 23, 31, Q16, seed=7) // 3 + 15000).astype(dtype)
    want = ref_auto_level(ref_image(refmod, px, mask="RGBA")).numpy()
    assert kept_channels_equal(want, px, [3])
    assert not np.array_equal(want[..., :3], px[..., :3])
    assert_same(min_max_stretch(px, (0, 1, 2, 3), False, 0.0, 0.0, 1.0), want, "auto-level mask RGBA")
    default = ref_auto_level(ref_image(refmod, px)).numpy()
    assert not np.array_equal(default[..., 3], px[..., 3])
    assert_same(min_max_stretch(px, (0, 1, 2, 3), True, 0.0, 0.0, 1.0), default, "auto-level default mask")
    gray = np.ascontiguousarray(px[..., [0, 3]])
    want = ref_auto_level(ref_image(refmod, gray, mask="RGBA")).numpy()
    assert kept_channels_equal(want, gray, [1])
    assert_same(min_max_stretch(gray, (0, 1), False, 0.0, 0.0, 1.0), want, "auto-level gray+alpha mask RGBA")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_linear_stretch_restatement(refmod, layout, dtype):
    frames = [("noise", frame(layout, 23, 31, dtype)), ("ramp", ramp(CHANNELS[layout], dtype))]
    if dtype == HDRI:
        frames.append(("out of range", out_of_range_float(23, 31, CHANNELS[layout])))
    for what, px in frames:
        pixels = px.shape[0] * px.shape[1]
        for black_point, white_point in ((0.0, 0.0), (0.02 * pixels, 0.01 * pixels), (pixels + 10.0, pixels + 10.0)):
            image, text = ref_linear_stretch(ref_image(refmod, px), black_point, white_point)
            got, black, white = linear_stretch(px, every(px), black_point, white_point)
            assert linear_stretch_property(black, white) == text, "%s %s %s" % (layout, what, (black_point, white_point))
            assert_same(got, image.numpy(), "linear-stretch %s %s %s" % (layout, what, (black_point, white_point)))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_two_compositions(refmod, layout, dtype):
    """NormalizeImage is ContrastStretchImage at 0.02 and 0.99 of the pixels; BrightnessContrastImage
    is FunctionImage(Polynomial) with slope and intercept."""
    px = frame(layout, 23, 31, dtype)
    pixels = px.shape[0] * px.shape[1]
    want = ref_normalize(ref_image(refmod, px)).numpy()
    assert_same(ref_image(refmod, px).contrast_stretch(0.02 * px.shape[1] * px.shape[0], 0.99 * px.shape[1] * px.shape[0]).numpy(),
                want, "normalize %s (%d pixels)" % (layout, pixels))
    for brightness, contrast in ((0.0, 0.0), (10.0, 20.0), (-15.0, -30.0), (5.0, 100.0), (0.0, -100.0)):
        coefficients = brightness_contrast_coefficients(brightness, contrast)
        want = ref_brightness_contrast(ref_image(refmod, px), brightness, contrast).numpy()
        assert_same(ref_image(refmod, px).function("Polynomial", coefficients).numpy(), want,
                    "brightness-contrast as FunctionImage %s %s" % (layout, (brightness, contrast)))
        assert_same(polynomial(px, every(px), coefficients), want, "brightness-contrast %s %s" % (layout, (brightness, contrast)))


@pytest.mark.parametrize("quantum,dtype", [(0, Q16), (1, HDRI)])
def test_gamma_lut_is_the_model(lib, quantum, dtype):
    for value in GAMMAS + [1.0e-13, -2.0]:
        assert np.array_equal(lib.gamma_lut(value, quantum), gamma_map(value, dtype)), "gamma %g" % value
