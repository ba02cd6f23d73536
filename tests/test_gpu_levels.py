"""The level operators (MagickCore/enhance.c, histogram.c) on the device, through the C ABI, against the
compiled reference.  Q16: every sample equal, in both precision modes.  Float Quantum: every sample
equal where no libm is involved (gamma == 1, NegateImage) and for GammaImage (table-driven in the
reference too); where the device's pow / tanh / atanh is, within one float ULP and at most 0.1 % of a
frame's samples different at all: an fp64 result an ulp or two off changes the rounded float only
within about 2^-29 of a rounding boundary, about 1e-8 of the samples, so 0.1 % is far above a
correct kernel and far below one that evaluates in single precision."""
import numpy as np
import pytest

from conftest import to_device, ulp_diff_f32
from statistic_oracle import assert_same
from levels_oracle import (CHANNELS, LAYOUTS, LEVELS, SIGMOIDALS, GAMMAS, MASKS, EPSILON, ref_image, ref_level,
                           ref_levelize, ref_gamma, ref_negate, ref_sigmoidal, ref_min_max_stretch, ref_auto_level,
                           ref_linear_stretch, ref_normalize, ref_brightness_contrast, ref_range,
                           linear_stretch_property, ramp, frame, gray_pixels, seed_frame, constant, out_of_range_float,
                           kept_channels_equal)

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED = 1
LIBM_SHARE = 1.0e-3
EDGES = [(1, 1), (1, 40), (40, 1)]                 # rows x columns
BIG = (1449, 1449)                                 # one trip of the point kernel's grid is 8192 x 256 pixels


def device_image(im, px, layout=None, host=False, **kw):
    alpha = (px.shape[2] in (2, 4)) if layout is None else layout in ("gray+alpha", "rgba")
    return im.Image(px.copy() if host else to_device(px), has_alpha=alpha, **kw)


def check(got, want, what, libm=False):
    """Bit for bit; with libm on float Quantum one ULP, and at most LIBM_SHARE of the samples different."""
    if not libm or want.dtype != np.float32:
        assert_same(got, want, what)
        return 0.0
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ" % what
    ulp = ulp_diff_f32(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0))
    share = float((ulp != 0).mean())
    print("%s: %d of %d samples differ (share %.3g), max %d ULP" % (what, int((ulp != 0).sum()), ulp.size, share, ulp.max()))
    assert ulp.max() <= 1, "%s: max ULP diff = %d, %d of %d over" % (what, ulp.max(), int((ulp > 1).sum()), ulp.size)
    assert share <= LIBM_SHARE, "%s: %.3g of the samples differ" % (what, share)
    return share


def level_libm(gamma):
    return 1.0 / gamma != 1.0 if abs(gamma) >= EPSILON else True


def run_pointwise(im, refmod, px, what, layout=None, mask=None, copy=(), host=False):
    """Every pointwise entry point on one frame.  mask: a name of MASKS (an RGBA frame)."""
    kw = {}
    if mask is not None:
        kw = {"channel_mask": MASKS[mask][0], "copy_channels": MASKS[mask][1]}
    elif copy:
        kw = {"copy_channels": copy}

    def image():
        return device_image(im, px, layout, host, **kw)

    def ref():
        if mask is None and copy:
            # a Copy channel under the default mask: the reference's mask that leaves it out
            assert px.shape[2] == 4 and tuple(copy) == (3,)
            return ref_image(refmod, px, mask="RGB")
        return ref_image(refmod, px, mask=mask)

    for black, white, gamma in LEVELS:
        tag = "%s %s" % ((black, white, gamma), what)
        check(im.level_image(image(), black, white, gamma).numpy(), ref_level(ref(), black, white, gamma).numpy(),
              "level " + tag, level_libm(gamma))
        check(im.levelize_image(image(), black, white, gamma).numpy(), ref_levelize(ref(), black, white, gamma).numpy(),
              "levelize " + tag, gamma != 1.0)
    for gamma in GAMMAS:
        check(im.gamma_image(image(), gamma).numpy(), ref_gamma(ref(), gamma).numpy(), "gamma %g %s" % (gamma, what))
    for grayscale in (False, True):
        check(im.negate_image(image(), grayscale).numpy(), ref_negate(ref(), grayscale).numpy(),
              "negate grayscale=%s %s" % (grayscale, what))
    for sharpen, contrast, midpoint in SIGMOIDALS:
        check(im.sigmoidal_contrast_image(image(), sharpen, contrast, midpoint).numpy(),
              ref_sigmoidal(ref(), sharpen, contrast, midpoint).numpy(),
              "sigmoidal %s %s" % ((sharpen, contrast, midpoint), what), True)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pointwise_on_the_full_ramp(im, refmod, layout, dtype):
    """All 65536 Q16 inputs, so every table entry is exercised."""
    px = ramp(CHANNELS[layout], dtype)
    if CHANNELS[layout] >= 3:
        px = gray_pixels(px)
    run_pointwise(im, refmod, px, "ramp %s %s" % (layout, px.dtype.name), layout)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pointwise_odd_frames(im, refmod, layout, dtype):
    px = frame(layout, 37, 53, dtype)
    if CHANNELS[layout] >= 3:
        px = gray_pixels(px)
    run_pointwise(im, refmod, px, "37x53 %s %s" % (layout, px.dtype.name), layout)
    for rows, cols in EDGES:
        run_pointwise(im, refmod, frame(layout, rows, cols, dtype, seed=1), "%dx%d %s" % (rows, cols, layout), layout)
    if dtype == HDRI:
        run_pointwise(im, refmod, out_of_range_float(37, 53, CHANNELS[layout]), "out of range %s" % layout, layout)


def test_float_sigmoidal_on_samples_at_the_curve_s_zero(im, refmod):
    """Reduced from stress family 24 (tests/stress_parity.py, seed 6024, cases #14, #84 and #1206): float alphas of
    exactly 0 and of 1e-9 ... 1e-4 under both sigmoidals.  There sig(x) - sig(0), and b + (2/a) atanh(...) in the inverse
    form, cancel to the last bits of tanh / atanh, where the device's libm and the host's differ: the device's results were
    up to 2.6e-11 off, 7.6e8 float ULPs of a result that small (7.85e-12 where the reference keeps an alpha of 0.0).  A
    sample of 0 now takes the host's constants and the other small ones the host's libm."""
    px = frame("rgba", 8, 8, HDRI, seed=21)
    px[..., 3] = (10.0 ** np.linspace(-9.0, -4.0, 64)).astype(np.float32).reshape(8, 8)
    px[0, :4, 3] = 0.0
    for sharpen, contrast, midpoint in [(1, 0.014478866124392493, 67587.2464210792), (1, 5.795376361120826, 15738.240882300885),
                                        (0, 13.991473358900219, 27437.970158007392)]:
        check(im.sigmoidal_contrast_image(device_image(im, px, "rgba"), sharpen, contrast, midpoint).numpy(),
              ref_sigmoidal(ref_image(refmod, px), sharpen, contrast, midpoint).numpy(),
              "sigmoidal %s, alpha 0 and 1e-9 ... 1e-4" % ((sharpen, contrast, midpoint),), True)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask", list(MASKS) + ["copy"])
def test_channel_masks_and_a_copy_channel(im, refmod, mask, dtype):
    px = gray_pixels(frame("rgba", 37, 53, dtype, seed=3))
    if mask == "copy":
        run_pointwise(im, refmod, px, "copy alpha %s" % px.dtype.name, "rgba", copy=(3,))
    else:
        run_pointwise(im, refmod, px, "mask %s %s" % (mask, px.dtype.name), "rgba", mask=mask)
        got = im.negate_image(device_image(im, px, channel_mask=MASKS[mask][0], copy_channels=MASKS[mask][1]), True).numpy()
        assert kept_channels_equal(got, px, MASKS[mask][1])


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_one_trip_past_the_grid(im, refmod, dtype):
    """1449 x 1449 RGBA: more pixels than one trip of the point kernel's grid, and past the million
    pixels from which a Q16 table is applied out of LDS; the range kernel walks many trips."""
    px = frame("rgba", BIG[0], BIG[1], dtype, seed=8)
    px[..., 3] = px[..., 3] // 2 + 9000 if dtype == Q16 else px[..., 3] / 2 + 9000
    what = "1449x1449 rgba %s" % px.dtype.name
    check(im.level_image(device_image(im, px), 12345.5, 40000.25, 1.0).numpy(),
          ref_level(ref_image(refmod, px), 12345.5, 40000.25, 1.0).numpy(), "level gamma 1 " + what)
    check(im.level_image(device_image(im, px), 5000.0, 60000.0, 2.2).numpy(),
          ref_level(ref_image(refmod, px), 5000.0, 60000.0, 2.2).numpy(), "level " + what, True)
    check(im.negate_image(device_image(im, px), False).numpy(), ref_negate(ref_image(refmod, px), False).numpy(),
          "negate " + what)
    check(im.sigmoidal_contrast_image(device_image(im, px), 0, 5.0, 32767.5).numpy(),
          ref_sigmoidal(ref_image(refmod, px), 0, 5.0, 32767.5).numpy(), "inverse sigmoidal " + what, True)
    assert im.image_range(device_image(im, px, channel_mask=MASKS["A"][0], copy_channels=MASKS["A"][1])) == \
        ref_range(ref_image(refmod, px, mask="A"))
    check(im.auto_level_image(device_image(im, px)).numpy(), ref_auto_level(ref_image(refmod, px)).numpy(),
          "auto-level " + what)


# ------------------------------------------------------------------------------------------- range
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("shape", [(37, 53), (300, 301), BIG])
def test_range_extremes(im, refmod, shape, dtype):
    """The extremes at the first pixel, the last pixel, inside the ragged tail of the last workgroup,
    and in column 0 of channel 0 with channel 0 outside the mask."""
    rows, cols = shape
    base = (frame("rgba", rows, cols, Q16, seed=12) // 4 + 20000).astype(dtype)
    tail = rows * cols - 1 - ((rows * cols) % 256) // 2          # inside the last, partial workgroup
    places = {"first": (0, 0), "last": (rows - 1, cols - 1), "tail": divmod(tail, cols), "middle": (rows // 2, cols // 3)}
    for where, (y, x) in places.items():
        for channel in (1, 3):
            px = base.copy()
            px[y, x, channel] = 65000
            px[rows - 1 - y, cols - 1 - x, channel] = 100
            got = im.image_range(device_image(im, px))
            assert got == ref_range(ref_image(refmod, px)), "%s channel %d %s" % (where, channel, shape)
            assert got == (100.0, 65000.0)
    for host in (False, True):
        px = base.copy()
        px[rows // 2, 0, 0] = 65100
        px[rows - 1, 0, 0] = 7
        px[rows // 3, cols - 1, 0] = 3                            # channel 0 away from column 0: outside the range
        for mask in ("A", "RGB", "R"):
            got = im.image_range(device_image(im, px, host=host, channel_mask=MASKS[mask][0], copy_channels=MASKS[mask][1]))
            assert got == ref_range(ref_image(refmod, px, mask=mask)), "seed, mask %s %s" % (mask, shape)
        assert im.image_range(device_image(im, px, host=host, channel_mask=MASKS["A"][0], copy_channels=MASKS["A"][1])) == \
            (7.0, 65100.0)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_range_of_every_layout(im, refmod, layout, dtype):
    frames = [frame(layout, rows, cols, dtype, seed=13) for rows, cols in [(37, 53)] + EDGES]
    frames += [np.zeros((5, 7, CHANNELS[layout]), dtype=dtype)]     # *maximum stays at MagickMinimumValue
    if dtype == HDRI:
        frames += [out_of_range_float(37, 53, CHANNELS[layout]), -np.abs(out_of_range_float(9, 11, CHANNELS[layout]))]
    for px in frames:
        assert im.image_range(device_image(im, px, layout)) == ref_range(ref_image(refmod, px)), "%s %s" % (layout, px.shape)


# --------------------------------------------------------------------------------- MinMaxStretchImage
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_min_max_stretch(im, refmod, layout, dtype):
    frames = [("narrow", (frame(layout, 37, 53, Q16, seed=14) // 3 + 9000).astype(dtype)),
              ("constant", constant(37, 53, CHANNELS[layout], dtype)), ("1x1", frame(layout, 1, 1, dtype)),
              ("40x1", (frame(layout, 40, 1, Q16) // 2 + 500).astype(dtype))]
    if dtype == HDRI:
        frames.append(("out of range", out_of_range_float(37, 53, CHANNELS[layout])))
    for what, px in frames:
        for black, white, gamma in ((0.0, 0.0, 1.0), (500.0, 1200.5, 1.0), (0.0, 0.0, 2.2), (300.0, 0.0, 0.45)):
            got = im.min_max_stretch_image(device_image(im, px, layout), black, white, gamma).numpy()
            want = ref_min_max_stretch(ref_image(refmod, px), black, white, gamma).numpy()
            check(got, want, "min-max %s %s %s %s" % ((black, white, gamma), layout, what, px.dtype.name), gamma != 1.0)
        check(im.auto_level_image(device_image(im, px, layout)).numpy(), ref_auto_level(ref_image(refmod, px)).numpy(),
              "auto-level %s %s" % (layout, what))
    got = im.auto_level_image(device_image(im, frames[1][1], layout)).numpy()
    assert_same(got, frames[1][1], "a constant frame is untouched")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("host", [False, True])
def test_min_max_stretch_per_channel(im, refmod, host, dtype):
    """The three properties of the reference that tests/test_levels_model.py pins, on the device."""
    def image(px, mask):
        return device_image(im, px, host=host, channel_mask=MASKS[mask][0], copy_channels=MASKS[mask][1])

    # 1. the seed: mask A of RGBA measures alpha and column 0 of red (and, per channel, levels nothing)
    px = (frame("rgba", 23, 31, Q16, seed=5) // 4 + 20000).astype(dtype)
    px[7, 0, 0], px[11, 0, 0], px[3, 5, 0] = 150, 64000, 10
    assert im.image_range(image(px, "A")) == ref_range(ref_image(refmod, px, mask="A")) == (150.0, 64000.0)
    check(im.auto_level_image(image(px, "A")).numpy(), ref_auto_level(ref_image(refmod, px, mask="A")).numpy(), "mask A")
    # 2. channel 0 is levelled before channel 1 is measured
    px = seed_frame(dtype)
    got = im.auto_level_image(device_image(im, px, host=host, channel_mask=MASKS["RGB"][0])).numpy()
    check(got, ref_auto_level(ref_image(refmod, px, mask="RGB")).numpy(), "mask RGB, extremes in column 0")
    assert kept_channels_equal(got, px, [1, 2]) and got[..., 0].min() == 0 and got[..., 0].max() == 65535
    # 3. 1 << offset is a ChannelType bit: alpha is never levelled per channel, it is under the default mask
    px = (frame("rgba", 37, 53, Q16, seed=7) // 3 + 15000).astype(dtype)
    rgba = MASKS["RGB"][0] | MASKS["A"][0]
    got = im.auto_level_image(device_image(im, px, host=host, channel_mask=rgba)).numpy()
    check(got, ref_auto_level(ref_image(refmod, px, mask="RGBA")).numpy(), "mask RGBA")
    assert kept_channels_equal(got, px, [3]) and not np.array_equal(got[..., :3], px[..., :3])
    got = im.auto_level_image(device_image(im, px, host=host)).numpy()
    check(got, ref_auto_level(ref_image(refmod, px)).numpy(), "default mask")
    assert not np.array_equal(got[..., 3], px[..., 3])
    gray = np.ascontiguousarray(px[..., [0, 3]])
    got = im.auto_level_image(device_image(im, gray, host=host, channel_mask=rgba)).numpy()
    check(got, ref_auto_level(ref_image(refmod, gray, mask="RGBA")).numpy(), "gray+alpha mask RGBA")
    assert kept_channels_equal(got, gray, [1])
    # per channel with a gamma: one table per channel on Q16
    got = im.min_max_stretch_image(device_image(im, px, host=host, channel_mask=MASKS["RGB"][0]), 200.0, 100.0, 2.2).numpy()
    check(got, ref_min_max_stretch(ref_image(refmod, px, mask="RGB"), 200.0, 100.0, 2.2).numpy(), "mask RGB gamma 2.2", True)


# --------------------------------------------------------- LinearStretch, Normalize, BrightnessContrast
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_linear_stretch(im, refmod, layout, dtype):
    frames = [("noise", frame(layout, 37, 53, dtype)), ("ramp", ramp(CHANNELS[layout], dtype))]
    if dtype == HDRI:
        frames.append(("out of range", out_of_range_float(37, 53, CHANNELS[layout])))
    for what, px in frames:
        pixels = px.shape[0] * px.shape[1]
        for black_point, white_point in ((0.0, 0.0), (0.02 * pixels, 0.01 * pixels), (pixels + 10.0, pixels + 10.0)):
            image, black, white = im.linear_stretch_image(device_image(im, px, layout), black_point, white_point)
            want, text = ref_linear_stretch(ref_image(refmod, px), black_point, white_point)
            assert linear_stretch_property(black, white) == text, "%s %s %s" % (layout, what, (black_point, white_point))
            check(image.numpy(), want.numpy(), "linear-stretch %s %s %s" % (layout, what, (black_point, white_point)))
    px = gray_pixels(frame("rgba", 37, 53, dtype, seed=4))
    image, black, white = im.linear_stretch_image(
        device_image(im, px, channel_mask=MASKS["RGB"][0], copy_channels=MASKS["RGB"][1]), 40.0, 20.0)
    want, text = ref_linear_stretch(ref_image(refmod, px, mask="RGB"), 40.0, 20.0)
    assert linear_stretch_property(black, white) == text
    check(image.numpy(), want.numpy(), "linear-stretch mask RGB")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_two_compositions(im, refmod, layout, dtype):
    px = frame(layout, 37, 53, dtype, seed=15)
    check(im.normalize_image(device_image(im, px, layout)).numpy(), ref_normalize(ref_image(refmod, px)).numpy(),
          "normalize %s %s" % (layout, px.dtype.name))
    for brightness, contrast in ((0.0, 0.0), (10.0, 20.0), (-15.0, -30.0), (5.0, 100.0), (0.0, -100.0)):
        check(im.brightness_contrast_image(device_image(im, px, layout), brightness, contrast).numpy(),
              ref_brightness_contrast(ref_image(refmod, px), brightness, contrast).numpy(),
              "brightness-contrast %s %s" % ((brightness, contrast), layout))


# ------------------------------------------------------------------- memory kinds, modes, the cache
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("host", [False, True])
def test_memory_kinds_and_precision_modes(im, refmod, host, dtype):
    px = gray_pixels(frame("rgba", 37, 53, dtype, seed=9))
    want = {"level": ref_level(ref_image(refmod, px), 5000.0, 60000.0, 2.2).numpy(),
            "level1": ref_level(ref_image(refmod, px), 5000.0, 60000.0, 1.0).numpy(),
            "levelize": ref_levelize(ref_image(refmod, px), 5000.0, 60000.0, 0.45).numpy(),
            "gamma": ref_gamma(ref_image(refmod, px), 2.2).numpy(),
            "negate": ref_negate(ref_image(refmod, px), True).numpy(),
            "sigmoidal": ref_sigmoidal(ref_image(refmod, px), 1, 5.0, 32767.5).numpy(),
            "autolevel": ref_auto_level(ref_image(refmod, px)).numpy(),
            "linear": ref_linear_stretch(ref_image(refmod, px), 40.0, 20.0)[0].numpy()}
    libm = {"level", "levelize", "sigmoidal"}
    try:
        for precision in (im.PRECISION_FAST, im.PRECISION_EXACT):
            im.set_precision(precision)
            new = lambda: device_image(im, px, host=host)        # noqa: E731
            got = {"level": im.level_image(new(), 5000.0, 60000.0, 2.2), "level1": im.level_image(new(), 5000.0, 60000.0, 1.0),
                   "levelize": im.levelize_image(new(), 5000.0, 60000.0, 0.45), "gamma": im.gamma_image(new(), 2.2),
                   "negate": im.negate_image(new(), True), "sigmoidal": im.sigmoidal_contrast_image(new(), 1, 5.0, 32767.5),
                   "autolevel": im.auto_level_image(new()), "linear": im.linear_stretch_image(new(), 40.0, 20.0)[0]}
            for name in want:
                check(got[name].numpy(), want[name], "%s host=%s precision %d" % (name, host, precision), name in libm)
    finally:
        im.set_precision(im.PRECISION_EXACT)


def test_table_cache(im, refmod):
    """A second call with the same parameters builds no table; a call with other parameters builds
    one; the results are right in either order."""
    px = ramp(4, Q16)
    first, second = (4321.5, 61234.25, 1.9), (4321.5, 61234.25, 0.6)
    want = {p: ref_level(ref_image(refmod, px), *p).numpy() for p in (first, second)}
    built = im.levels_tables_built()
    check(im.level_image(device_image(im, px), *first).numpy(), want[first], "first parameters")
    assert im.levels_tables_built() == built + 1
    check(im.level_image(device_image(im, px), *first).numpy(), want[first], "first parameters again")
    assert im.levels_tables_built() == built + 1
    check(im.level_image(device_image(im, px), *second).numpy(), want[second], "second parameters")
    assert im.levels_tables_built() == built + 2
    check(im.level_image(device_image(im, px), *first).numpy(), want[first], "first parameters after the second")
    check(im.level_image(device_image(im, px), *second).numpy(), want[second], "second parameters again")
    assert im.levels_tables_built() == built + 2
    # the same numbers in another operator are another table
    check(im.levelize_image(device_image(im, px), *first).numpy(), ref_levelize(ref_image(refmod, px), *first).numpy(),
          "levelize with the first parameters")
    assert im.levels_tables_built() == built + 3


# --------------------------------------------------------------------------------- batch and sharded
def direct(im, px, chain):
    calls = {"level": im.level_image, "levelize": im.levelize_image, "gamma": im.gamma_image, "negate": im.negate_image,
             "sigmoidalcontrast": im.sigmoidal_contrast_image, "autolevel": im.auto_level_image,
             "normalize": im.normalize_image, "blur": im.blur_image,
             "linearstretch": lambda image, black, white: im.linear_stretch_image(image, black, white)[0]}
    image = im.Image(to_device(px), precision=im.PRECISION_EXACT)
    for step in chain:
        image = calls[step[0]](image, *step[1:])
    return image.numpy()


CHAINS = [[("level", 5000.0, 60000.0, 2.2), ("blur", 0.0, 1.0), ("negate", 0)],
          [("levelize", 3000.0, 50000.0, 0.45), ("gamma", 2.2), ("negate", 1)],
          [("sigmoidalcontrast", 1, 5.0, 32767.5), ("sigmoidalcontrast", 0, 5.0, 32767.5)],
          [("autolevel",), ("linearstretch", 40.0, 20.0)], [("normalize",)]]


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("chain", CHAINS, ids=lambda chain: "+".join(step[0] for step in chain))
def test_batch_equals_the_calls_one_by_one(im, chain, memory, dtype):
    for channels in (1, 4, 3, 2):
        p = frame(LAYOUTS[channels - 1], 48, 64, dtype, seed=900 + channels)
        image = im.Image(p.copy() if memory == "host" else to_device(p), precision=im.PRECISION_EXACT)
        result = image.like()
        report = im.batch_images(chain, [image], [result], devices=2, streams_per_device=2)
        assert sum(report["images_per_device"]) == 1
        assert_same(result.numpy(), direct(im, p, chain), "batch %s (%s, %d channels)" % (chain, memory, channels))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("chain", CHAINS[:3], ids=lambda chain: "+".join(step[0] for step in chain))
def test_sharded_equals_the_unsharded_call(im, chain, dtype):
    px = gray_pixels(frame("rgba", 80, 96, dtype, seed=61))
    result, report = im.sharded_image(chain, im.Image(px.copy(), precision=im.PRECISION_EXACT), devices=2)
    assert report["devices"] == 2
    assert_same(result.numpy(), direct(im, px, chain), "sharded %s" % (chain,))


@pytest.mark.parametrize("chain", [[("autolevel",)], [("linearstretch", 40.0, 20.0)], [("normalize",)],
                                   [("negate", 0), ("autolevel",)]], ids=lambda chain: chain[-1][0])
def test_sharded_range_operators_are_declined_untouched(im, chain):
    px = frame("rgba", 80, 96, Q16, seed=62)
    image, result = im.Image(px.copy()), im.Image(np.full_like(px, 77))
    with pytest.raises(im.MagickHipError) as error:
        im.sharded_image(chain, image, result, devices=2)
    assert error.value.status == MH_UNSUPPORTED
    assert np.array_equal(image.numpy(), px) and np.array_equal(result.numpy(), np.full_like(px, 77))
