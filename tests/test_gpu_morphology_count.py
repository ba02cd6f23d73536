"""The number MagickHipMorphologyPrimitive returns — how many samples one pass changed — against the fp64
restatement of tests/morphology_oracle.py (checked by hand in test_morphology_count_model.py), and the pixels of
the same call against the compiled reference.

The reference counts |pixel - sample| >= MagickEpsilon on the UNROUNDED result (morphology.c:2772, :3199) and
divides by the channels that carry the update trait (:2806, :3226).  The compiled reference does not hand the
number out, so the inputs are such that it does not depend on the summation order: integer cells, integer samples,
biases that are multiples of 1/4 — every partial sum is exact in fp64.

Found with these tests, fixed in operators.cpp:
  * a one-channel Q16 Convolve took the four-row-band route whatever `changed` was and counted "rounded level !=
    source level" while unpacking: the identity kernel with a bias of 0.25 on a 37 x 45 frame returned 0 where the
    reference counts all 1665 samples, unnormalised 1,2,1 2,4,2 1,2,1 returned 1456 for 1585 (clamped sums).
    The route is now taken only when no count is wanted, like every other fast Convolve route.
  * the count was divided by the pixel's width, not by the channels that carry the update trait: three channels of
    which one is masked returned 2/3 of the reference's number — 1110 for 1665 on the same frame under -channel RB —
    and an iteration "until nothing changes" ended as soon as a pass changed fewer samples than the pixel has channels."""
import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity
from morphology_oracle import changed_count

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
ROWS, COLS = 37, 45

IDENTITY = "3x3: 0,0,0 0,1,0 0,0,0"
BINOMIAL = "3x3: 1,2,1 2,4,2 1,2,1"
CONVOLVE_CASES = [(IDENTITY, 0.0), (IDENTITY, 0.25), (BINOMIAL, 0.0), (BINOMIAL, -0.75),
                  ("5x1: 1,2,3,2,1", 0.0), ("1x5: 1,2,3,2,1", 0.0), ("5x1+1+0: -1,2,3,2,-1", 0.5),
                  ("1x5+0+3: 1,0,-2,0,1", 0.0), ("5x1: 0,0,1,0,0", 0.0), ("1x5: 0,0,1,0,0", 0.25)]
MINMAX_KERNELS = ["Disk:3", "Square:1", "Rectangle:5x3+1+1"]


def frame(channels, dtype, seed=5):
    """Integer samples (float Quantum too), some of them at 65535, and a constant patch at 0: there a clamped
    result equals the source level while the unrounded sum does not — and the sum over the patch's middle does."""
    rng = np.random.default_rng(seed + channels)
    px = rng.integers(0, 65536, (ROWS, COLS, channels), dtype=np.uint16)
    px[rng.random((ROWS, COLS, channels)) < 0.05] = 65535
    px[3:9, 30:41] = 65535
    px[20:30, 5:17] = 0
    return np.ascontiguousarray(px.astype(dtype))


def reference_pixels(refmod, px, method, kernel, bias, channels, mask=None):
    def run(pixels):
        ref = refmod.RefImage(pixels)
        if mask:
            ref.set_channel_mask(mask)
        if bias != 0.0:
            ref.set_artifact("convolve:bias", "%.17g" % bias)
        return ref.morphology(method, 1, kernel).numpy()
    if channels == 4:                                    # four plain channels: each one on its own
        return np.concatenate([run(px[:, :, c].copy()).reshape(ROWS, COLS, 1) for c in range(4)], axis=2)
    return run(px).reshape(px.shape)


def check(im, refmod, px, method, kernel, bias, channels, what, copy_channels=(), mask=None):
    values, x, y, _ = refmod.kernel(kernel)
    samples, want = changed_count(px, method, values, x, y, bias, copy_channels)
    dev = im.Image(to_device(px), has_alpha=False, copy_channels=copy_channels)
    out, got = im.morphology_primitive(dev, method, kernel, bias)
    print("%s: library %d, restatement %d (%d samples)" % (what, got, want, samples))
    assert got == want, "%s: the library counts %d, the reference %d (%d samples of %d)" % (
        what, got, want, samples, px.size)
    assert_parity(out.numpy(), reference_pixels(refmod, px, method, kernel, bias, channels, mask), True, what)
    return samples


DTYPES = pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
MASK_CASES = [("Convolve", IDENTITY, 0.25), ("Convolve", BINOMIAL, 0.0), ("Convolve", "5x1: 1,2,3,2,1", 0.0),
              ("Convolve", "1x5: 1,2,3,2,1", 0.5), ("Erode", "Disk:3", 0.0), ("Dilate", "Rectangle:5x3+1+1", 0.0)]


@DTYPES
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_convolve_change_count(im, refmod, channels, dtype):
    px = frame(channels, dtype)
    for kernel, bias in CONVOLVE_CASES:
        what = "Convolve %s bias %g, %d channels %s" % (kernel, bias, channels, np.dtype(dtype).name)
        samples = check(im, refmod, px, "Convolve", kernel, bias, channels, what)
        if kernel == IDENTITY or kernel.endswith("0,0,1,0,0"):
            assert samples == (0 if bias == 0.0 else px.size), what
        elif kernel == BINOMIAL and bias == 0.0:
            # the samples at 65535 come back at 65535 (clamped) and count; the middle of the patch at 0 does not
            assert samples == px.size - 8 * 10 * channels, what


def test_convolve_change_count_with_the_gray_bands_switched_on(im, refmod, options):
    """One Q16 channel, the four-row-band form admitted for a frame this small: a pass that has to count does
    not take it (it would see levels, not sums), one that does not still does."""
    import bench
    options.set("MAGICKHIP_GRAY_BANDS_MIN_PIXELS", "0")
    px = frame(1, Q16)
    dev = im.Image(to_device(px))
    for kernel, bias in CONVOLVE_CASES:
        what = "Convolve %s bias %g, gray bands admitted" % (kernel, bias)
        samples = check(im, refmod, px, "Convolve", kernel, bias, 1, what)
        if kernel == IDENTITY:
            assert samples == (0 if bias == 0.0 else ROWS * COLS), what
        counted = set(bench.kernel_profile(im, lambda: im.morphology_primitive(dev, "Convolve", kernel, bias), 1))
        assert "gray_bands_pack" not in counted, (what, counted)
        if kernel.startswith("3x3"):
            holder = {}
            launched = set(bench.kernel_profile(
                im, lambda: holder.update(out=im.morphology_image(dev, "Convolve", 1, kernel, bias=bias)), 1))
            assert {"gray_bands_pack", "gray_bands_unpack"} <= launched, (what, launched)
            assert_parity(holder["out"].numpy(), reference_pixels(refmod, px, "Convolve", kernel, bias, 1), True,
                          what + " (no count: the band form)")


@DTYPES
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_erode_dilate_change_count(im, refmod, channels, dtype, options):
    px = frame(channels, dtype)
    cases = [(method, kernel) for method in ("Erode", "Dilate") for kernel in MINMAX_KERNELS]
    for method, kernel in cases:
        what = "%s %s, %d channels %s" % (method, kernel, channels, np.dtype(dtype).name)
        samples = check(im, refmod, px, method, kernel, 0.0, channels, what)
        assert 0 < samples < px.size, what
    if channels == 1 and dtype is Q16:
        options.set("MAGICKHIP_GRAY_BANDS_MIN_PIXELS", "0")     # the band form counts exact sample values: it stays
    elif channels == 3:
        options.set("MAGICKHIP_RGB_PAD_MIN_PIXELS", "0")          # ... and so does RGB padded to four channels
        options.set("MAGICKHIP_RGB_PAD_FLOAT_ALWAYS", "1")
    else:
        return
    for method, kernel in cases:
        check(im, refmod, px, method, kernel, 0.0, channels, "%s %s, %d channels %s, wide-pixel form admitted" % (
            method, kernel, channels, np.dtype(dtype).name))


@DTYPES
def test_change_count_with_a_channel_mask(im, refmod, dtype, options):
    """-channel RB on three channels: green comes back bit for bit and does not count, and the count is divided by
    the two channels that carry the update trait (GetImageChannels), not by the pixel's three."""
    px = frame(3, dtype, seed=11)
    for method, kernel, bias in MASK_CASES:
        what = "%s %s bias %g -channel RB, %s" % (method, kernel, bias, np.dtype(dtype).name)
        samples = check(im, refmod, px, method, kernel, bias, 3, what, copy_channels=(1,), mask="RB")
        if kernel == IDENTITY:
            assert samples == 2 * ROWS * COLS, what
    options.set("MAGICKHIP_RGB_PAD_MIN_PIXELS", "0")
    options.set("MAGICKHIP_RGB_PAD_FLOAT_ALWAYS", "1")
    for method, kernel, bias in MASK_CASES[4:]:
        check(im, refmod, px, method, kernel, bias, 3, "%s %s -channel RB, padded, %s" % (method, kernel, np.dtype(dtype).name),
              copy_channels=(1,), mask="RB")


@DTYPES
def test_unbounded_iteration_with_a_channel_mask_runs_until_nothing_changes(im, refmod, dtype):
    """What the divisor decides: Erode with `2x1+0+0: 1,1` takes one pixel a pass off the right end of a
    one-pixel line — two samples under -channel RB, a count of 2/2 = 1 in the reference, which goes on until the
    line is gone.  Divided by the pixel's three channels the count is 0 and the iteration ends after its first pass."""
    px = np.zeros((ROWS, COLS, 3), dtype=dtype)
    px[5, 3:13] = 65535
    px[20:23, 30] = 65535
    want = refmod.RefImage(px).set_channel_mask("RB").morphology("Erode", -1, "2x1+0+0: 1,1").numpy()
    assert not want[:, :, (0, 2)].any() and np.array_equal(want[:, :, 1], px[:, :, 1])
    dev = im.Image(to_device(px), copy_channels=(1,))
    assert_parity(im.morphology_image(dev, "Erode", -1, "2x1+0+0: 1,1").numpy(), want, True, "Erode until stable, -channel RB")
