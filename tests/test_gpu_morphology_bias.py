"""Convolve / Correlate with a bias (`-define convolve:bias=`, the `bias` argument of MagickHipMorphologyImage*)
against the compiled reference.

A bias switches every fast Convolve route of primitive() off (operators.cpp) and sends the call to code with
arithmetic of its own: the 1-D vector kernels seed their accumulators with it (convolve.hip), the FAST f32 epilogue
of alpha-weighted frames forms (bias*QuantumRange + S_c)/S_a, the generic kernel seeds s[c] (morphology.hip), the
four-row-band form of a gray frame hands it to the wide-pixel call.  The reference seeds `pixel=bias` BEFORE the
alpha weighting (morphology.c:2740, :2899) and stores gamma*pixel: on alpha-weighted channels the bias is scaled by
1/sum(k*alpha) — by PerceptibleReciprocal(0) = 1e12 over a fully transparent window.

Contract (README, conftest.assert_parity): EXACT bit-identical on both Quantum types, FAST within one level on
Q16 and within one float ULP on float Quantum (the residue of a cancellation agrees absolutely: the allowance the
FAST float ResizeImage tests use)."""
import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
BIASES = [1000.0, -1000.0, 0.25, 32768.0, -70000.0]
RESIDUE = 65535.0e-9                                     # as test_resize_fast_intermediate_on_rounding_boundaries


def taps(n):
    """n normalised taps, not quite symmetric."""
    w = [(i + 1.0) * (n - i) + (i % 3) for i in range(n)]
    return ",".join("%.17g" % (v / sum(w)) for v in w)


# (kernel, normalise): 1-D in both directions, tap counts on either side of the launcher's 16-tap split, BlurImage's
# 79 taps, cells of both signs, an origin off centre
KERNELS_1D = [("3x1: 0.25,0.5,0.25", False), ("1x3: 0.25,0.5,0.25", False),
              ("15x1: " + taps(15), False), ("1x15: " + taps(15), False),
              ("17x1: " + taps(17), False), ("1x17: " + taps(17), False),
              ("blur:0x10", False), ("blur:0x10+90", False),
              ("5x1: -0.2,0.4,0.6,0.4,-0.2", False), ("1x5: -0.2,0.4,0.6,0.4,-0.2", False),
              ("5x1+1+0: 0.1,0.3,0.3,0.2,0.1", False), ("1x5+0+3: 0.1,0.3,0.3,0.2,0.1", False)]
ASYMMETRIC = "5x3+0+2: 0.1,0.2,-0.1,0.15,0.05 0,0.3,0,-0.2,0.1 -0.05,0.2,0.25,0.1,-0.1"
WITH_NAN = "3x3: 0.1,nan,0.2 nan,0.4,0.05 0.15,0.1,nan"
KERNELS_2D = [("3x3: 1,2,1 2,4,2 1,2,1", False), ("3x3: 1,2,1 2,4,2 1,2,1", True), ("Gaussian:0x1.5", False),
              ("Disk:3", False), ("Disk:3", True), (ASYMMETRIC, False), (WITH_NAN, False), (WITH_NAN, True)]
KERNELS_SMALL_FRAMES = [k for k in KERNELS_1D if k[0].startswith(("15x1", "1x15", "17x1", "1x17"))] + KERNELS_2D
LAYOUTS = ["gray", "graya", "rgb", "rgba", "plain4"]
CHANNELS = {"gray": 1, "graya": 2, "rgb": 3, "rgba": 4, "plain4": 4}


def reference(refmod, px, layout, method, kernel, normalise, bias, mask=None):
    def run(pixels):
        ref = refmod.RefImage(pixels)
        if mask:
            ref.set_channel_mask(mask)
        if normalise:
            ref.set_artifact("convolve:scale", "!")
        ref.set_artifact("convolve:bias", bias if isinstance(bias, str) else "%.17g" % bias)
        return ref.morphology(method, 1, kernel).numpy()
    if layout == "plain4":                               # four channels without alpha: each one on its own
        return np.concatenate([run(px[:, :, c].copy()).reshape(px.shape[0], px.shape[1], 1) for c in range(4)], axis=2)
    return run(px).reshape(px.shape)


def compare(got, want, exact, what):
    """assert_parity under the contract; on float frames the NaN pattern must match and the rest is compared."""
    is_float = want.dtype == np.float32
    if is_float:
        assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern differs" % what
        got, want = np.nan_to_num(got, nan=0.0, posinf=np.inf, neginf=-np.inf), \
            np.nan_to_num(want, nan=0.0, posinf=np.inf, neginf=-np.inf)
    if exact:
        assert_parity(got, want, True, what)
    else:
        assert_parity(got, want, False, what, max_ulp=1, residue=RESIDUE if is_float else 0.0)


def check(im, refmod, px, layout, kernels, biases=BIASES, method="Convolve", copy_channels=(), mask=None, what=""):
    """Every kernel x bias, EXACT and FAST, against the reference."""
    dev = im.Image(to_device(px), has_alpha=layout in ("graya", "rgba"), copy_channels=copy_channels)
    for kernel, normalise in kernels:
        for bias in biases:
            want = reference(refmod, px, layout, method, kernel, normalise, bias, mask)
            for precision, exact in ((im.PRECISION_EXACT, True), (im.PRECISION_FAST, False)):
                im.set_precision(precision)
                try:
                    got = im.morphology_image(dev, method, 1, kernel, bias=bias,
                                              scale=(1.0, 1) if normalise else None).numpy()
                finally:
                    im.set_precision(im.PRECISION_EXACT)
                compare(got.reshape(px.shape), want, exact, "%s %s%s bias %g, %s %s %s%s" % (
                    method, kernel[:24], "!" if normalise else "", bias, layout, np.dtype(px.dtype).name,
                    "EXACT" if exact else "FAST", what))


def random_frame(shape, layout, dtype, seed=0):
    return make_pixels(shape[0], shape[1], CHANNELS[layout], dtype, seed=seed + 7 * CHANNELS[layout] + shape[0])


DTYPES = pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])


@DTYPES
@pytest.mark.parametrize("layout", LAYOUTS)
def test_convolve_bias_1d(im, refmod, layout, dtype):
    check(im, refmod, random_frame((41, 57), layout, dtype), layout, KERNELS_1D)


@DTYPES
@pytest.mark.parametrize("layout", LAYOUTS)
def test_convolve_bias_2d(im, refmod, layout, dtype, options):
    import bench
    px = random_frame((41, 57), layout, dtype, seed=1)
    check(im, refmod, px, layout, KERNELS_2D)
    if layout == "gray" and dtype is Q16:
        # once more as four row bands (operators.cpp primitive()): the wide-pixel call inside carries the bias
        options.set("MAGICKHIP_GRAY_BANDS_MIN_PIXELS", "0")
        dev = im.Image(to_device(px))
        for kernel in KERNELS_2D:
            values, x, y, _ = im.kernel_to_numpy(kernel[0])
            launched = set(bench.kernel_profile(im, lambda: im.morphology_image(dev, "Convolve", 1, kernel[0], bias=0.25), 1))
            if (41 + 3) // 4 >= 2 * max(y, values.shape[0] - 1 - y):
                assert {"gray_bands_pack", "gray_bands_unpack"} <= launched, (kernel, launched)
        check(im, refmod, px, layout, KERNELS_2D, what=", as four row bands")


@DTYPES
def test_correlate_bias_asymmetric_kernel(im, refmod, dtype):
    for layout in LAYOUTS:
        px = random_frame((41, 57), layout, dtype, seed=2)
        check(im, refmod, px, layout, [(ASYMMETRIC, False)], method="Correlate")
        dev = im.Image(to_device(px), has_alpha=layout in ("graya", "rgba"))
        assert not np.array_equal(im.morphology_image(dev, "Correlate", 1, ASYMMETRIC, bias=0.25).numpy(),
                                  im.morphology_image(dev, "Convolve", 1, ASYMMETRIC, bias=0.25).numpy()), layout


def adversarial_frame(kind, layout, dtype):
    """(pixels, biases) of an alpha-weighted frame on which a bias goes wrong quietly."""
    rows, cols, channels = 41, 57, CHANNELS[layout]
    rng = np.random.default_rng(23 + channels)
    px = rng.integers(0, 65536, (rows, cols, channels), dtype=np.uint16)
    if kind == "sprite":
        # opaque rectangles on a fully transparent ground: windows with sum(k*alpha) = 0 put bias*1e12 at a clamp
        px[:, :, -1] = 0
        for y, x, h, w in ((4, 5, 9, 12), (20, 30, 1, 1), (25, 8, 13, 2), (30, 40, 8, 15), (12, 44, 3, 3)):
            px[y: y + h, x: x + w, -1] = 65535
        return px.astype(dtype), BIASES
    if kind == "tiny alpha":
        px[:, :, -1] = rng.integers(0, 4, (rows, cols), dtype=np.uint16)           # as stress_parity.pixels(kind=2)
        return px.astype(dtype), BIASES
    # a negative bias that all but cancels the weighted sum of a constant frame
    colour, alpha = 40000, 30000
    px[:, :, :-1] = colour
    px[:, :, -1] = alpha
    return px.astype(dtype), [round(-colour * alpha / 65535.0, 3)] + BIASES[:3]


@DTYPES
@pytest.mark.parametrize("kind", ["sprite", "tiny alpha", "cancelling bias"], ids=["sprite", "tiny", "cancel"])
def test_convolve_bias_alpha_weighted_adversarial_frames(im, refmod, kind, dtype):
    for layout in ("rgba", "graya"):
        px, biases = adversarial_frame(kind, layout, dtype)
        check(im, refmod, px, layout, KERNELS_1D + KERNELS_2D, biases, what=", " + kind)


@DTYPES
@pytest.mark.parametrize("shape", [(1, 40), (40, 1), (3, 5), (2, 2)], ids=["1x40", "40x1", "3x5", "2x2"])
def test_convolve_bias_frames_smaller_than_the_kernel(im, refmod, shape, dtype):
    for layout in LAYOUTS:
        check(im, refmod, random_frame(shape, layout, dtype, seed=3), layout, KERNELS_SMALL_FRAMES,
              what=", frame %dx%d" % shape)


def test_convolve_bias_percent_convention(im, refmod):
    """A plain number in convolve:bias is in Quantum units; a percentage is of QuantumRange + 1
    (StringToDoubleInterval, morphology.c:4171)."""
    px = random_frame((41, 57), "rgb", Q16, seed=4)
    want = reference(refmod, px, "rgb", "Convolve", "Gaussian:0x1.5", False, "25%")
    assert np.array_equal(want, reference(refmod, px, "rgb", "Convolve", "Gaussian:0x1.5", False, 0.25 * 65536))
    got = im.morphology_image(im.Image(to_device(px)), "Convolve", 1, "Gaussian:0x1.5", bias=0.25 * 65536).numpy()
    assert_parity(got, want, True, "convolve:bias=25%")


@DTYPES
def test_convolve_bias_with_a_channel_mask(im, refmod, dtype):
    """-channel RB on RGBA: green and alpha come back bit for bit, red and blue stay alpha-weighted."""
    px = random_frame((41, 57), "rgba", dtype, seed=5)
    kernels = [KERNELS_1D[2], KERNELS_1D[5], KERNELS_1D[8], KERNELS_2D[2], KERNELS_2D[5]]
    check(im, refmod, px, "rgba", kernels, copy_channels=(1, 3), mask="RB", what=", -channel RB")
    out = im.morphology_image(im.Image(to_device(px), copy_channels=(1, 3)), "Convolve", 1, kernels[0][0], bias=1000.0).numpy()
    assert np.array_equal(out[:, :, 1], px[:, :, 1]) and np.array_equal(out[:, :, 3], px[:, :, 3])


@DTYPES
def test_bias_is_ignored_outside_convolve(im, refmod, dtype):
    """morphology.c reads the bias inside the Convolve case only."""
    cases = [("Erode", "Disk:3"), ("Dilate", "Rectangle:5x3+1+1"), ("Open", "Disk:2.5"), ("EdgeIn", "Diamond:2"),
             ("Erode", "3x3: 1,nan,1 0.2,1,0.7 nan,1,0")]
    for layout in ("gray", "rgb", "rgba"):
        px = random_frame((41, 57), layout, dtype, seed=6)
        dev = im.Image(to_device(px))
        for method, kernel in cases:
            want = refmod.RefImage(px).set_artifact("convolve:bias", "1000").morphology(method, 1, kernel).numpy().reshape(px.shape)
            assert np.array_equal(want, refmod.RefImage(px).morphology(method, 1, kernel).numpy().reshape(px.shape))
            for precision in (im.PRECISION_EXACT, im.PRECISION_FAST):
                im.set_precision(precision)
                try:
                    biased = im.morphology_image(dev, method, 1, kernel, bias=1000.0).numpy()
                    plain = im.morphology_image(dev, method, 1, kernel).numpy()
                finally:
                    im.set_precision(im.PRECISION_EXACT)
                assert_parity(biased, want, True, "%s %s with a bias, %s, precision %d" % (method, kernel, layout, precision))
                assert_parity(plain, want, True, "%s %s, %s, precision %d" % (method, kernel, layout, precision))
