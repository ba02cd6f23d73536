"""AdaptiveThresholdImage (threshold.c:182-361) on the device against the compiled reference: every
sample equal on Q16 (exact integer window sums) and on float Quantum (the reference's running sum,
statement for statement), in both precision modes."""
import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from threshold_oracle import (kept_channels_equal, SHAPES, LAYOUTS, CHANNELS, MASKS, ref_image, ref_adaptive_threshold, frame, noise, constant,
                              flat_blocks, step_edge, wide_range_float, out_of_range_float)

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED = 1
# threshold.hip: input columns of a strip (it keeps SPAN-(W-1) output columns), rows of a band
# (max(BAND_ROWS, 4*H)), the widest Q16 window; further down the longest side of a float window
ADAPTIVE_SPAN = 512
ADAPTIVE_BAND_ROWS = 64
ADAPTIVE_MAX_WIDTH = 257
WINDOWS = [(1, 1), (1, 9), (9, 1), (2, 2), (4, 6), (3, 3), (7, 7), (16, 16), (25, 25), (64, 3), (3, 64)]
BIASES = [0.0, -0.25, 0.25, -1966.05, 1966.05, -70000.0, 70000.0]
ALL_SHAPES = SHAPES + [(16, 16), (17, 33)]


def check(im, refmod, px, width, height, bias, what="", **kw):
    got = im.adaptive_threshold_image(im.Image(to_device(px), **kw), width, height, bias).numpy()
    want = ref_adaptive_threshold(refmod, ref_image(refmod, px), width, height, bias).numpy()
    assert_same(got, want, "adaptive %dx%d%+g %s %s %s" % (width, height, bias, px.shape, px.dtype.name, what))
    return got


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_windows_and_biases(im, refmod, shape, dtype):
    """Every window on every shape; the layout and the bias step through their lists."""
    index = ALL_SHAPES.index(shape)
    for i, (width, height) in enumerate(WINDOWS):
        layout = LAYOUTS[(index + i) % len(LAYOUTS)]
        px = frame(layout, shape[0], shape[1], dtype, seed=i)
        check(im, refmod, px, width, height, BIASES[(index + 2 * i) % len(BIASES)], layout,
              has_alpha=layout in ("gray+alpha", "rgba"))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("bias", BIASES)
def test_every_bias(im, refmod, bias, dtype):
    px = frame("rgba", 61, 97, dtype, seed=11)
    got = check(im, refmod, px, 7, 7, bias)
    if abs(bias) == 70000.0:
        assert (got == (0 if bias > 0 else 65535)).all(), "all one value"


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_windows_larger_than_the_frame(im, refmod, dtype):
    check(im, refmod, frame("rgb", 15, 17, dtype), 41, 41, -0.25)
    check(im, refmod, frame("gray+alpha", 130, 70, dtype), 257, 257, 0.25)
    check(im, refmod, frame("gray", 130, 70, dtype), ADAPTIVE_MAX_WIDTH, 3, 0.0)


def test_more_than_two_strips_and_bands(im, refmod):
    """One column wider than two strips, one row taller than two bands."""
    width = height = 7
    columns = 2 * (ADAPTIVE_SPAN - (width - 1)) + 1
    rows = 2 * max(ADAPTIVE_BAND_ROWS, 4 * height) + 1
    check(im, refmod, noise(rows, columns, 1, Q16, seed=21), width, height, -0.25, "strips and bands")
    width, height = 64, 25
    columns = 2 * (ADAPTIVE_SPAN - (width - 1)) + 1
    rows = 2 * max(ADAPTIVE_BAND_ROWS, 4 * height) + 1
    check(im, refmod, noise(rows, columns, 2, Q16, seed=22), width, height, 655.35, "strips and bands")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 4])
def test_constant_frames_tie(im, refmod, channels, dtype):
    """N*v/N == v: with bias 0 the comparison is a tie everywhere, with -0.25 it fails everywhere."""
    px = constant(61, 97, channels, dtype)
    for width, height in [(3, 3), (7, 7), (4, 6), (25, 25), (64, 3)]:
        assert (check(im, refmod, px, width, height, 0.0, "constant") == 0).all()
        assert (check(im, refmod, px, width, height, -0.25, "constant") == 65535).all()


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_flat_blocks_and_step_edge(im, refmod, dtype):
    for what, px in (("flat blocks", flat_blocks(61, 97, 3, dtype)), ("step edge", step_edge(61, 97, 2, dtype))):
        for width, height, bias in [(3, 3, 0.0), (7, 7, -0.25), (16, 16, 0.25), (25, 25, 0.0), (4, 6, 1966.05)]:
            check(im, refmod, px, width, height, bias, what)


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_float_sums_carry_their_rounding_along_the_row(im, refmod, channels):
    """Samples of 1e-3 ... 6e4 in one frame, and samples outside the Quantum range: the order of the
    adds and the rounding carried from column 0 decide the last bits of the mean."""
    for what, px in (("wide range", wide_range_float(33, 131, channels)), ("out of range", out_of_range_float(33, 131, channels))):
        for width, height, bias in [(3, 3, 0.0), (7, 7, 0.0), (4, 6, -0.25), (25, 25, 0.25), (64, 3, 0.0), (3, 64, 0.0)]:
            check(im, refmod, px, width, height, bias, what)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask", list(MASKS))
def test_copy_channels_receive_the_centre_sample(im, refmod, mask, dtype):
    bits, copied = MASKS[mask]
    px = frame("rgba", 61, 97, dtype, seed=13)
    got = im.adaptive_threshold_image(im.Image(to_device(px), channel_mask=bits, copy_channels=copied), 7, 5, -0.25).numpy()
    want = ref_adaptive_threshold(refmod, ref_image(refmod, px, mask=mask), 7, 5, -0.25).numpy()
    assert_same(got, want, "mask %s" % mask)
    assert kept_channels_equal(got, px, copied)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("host", [False, True])
def test_memory_kinds_precision_modes_and_empty_windows(im, refmod, host, dtype):
    px = frame("rgba", 61, 97, dtype, seed=15)
    want = ref_adaptive_threshold(refmod, ref_image(refmod, px), 9, 7, 0.25).numpy()
    try:
        for precision in (im.PRECISION_FAST, im.PRECISION_EXACT):
            im.set_precision(precision)
            got = im.adaptive_threshold_image(im.Image(px.copy() if host else to_device(px)), 9, 7, 0.25).numpy()
            assert_same(got, want, "host=%s precision %d" % (host, precision))
    finally:
        im.set_precision(im.PRECISION_EXACT)
    for width, height in [(0, 5), (5, 0), (0, 0)]:
        got = im.adaptive_threshold_image(im.Image(px.copy() if host else to_device(px)), width, height, 0.0).numpy()
        assert_same(got, px, "width or height 0: a copy")
        assert_same(got, ref_adaptive_threshold(refmod, ref_image(refmod, px), width, height, 0.0).numpy(), "copy")


ADAPTIVE_FLOAT_MAX_SIDE = 1 << 20


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("host", [False, True])
def test_a_window_over_the_limit_is_declined_untouched(im, host, dtype):
    px = frame("rgb", 40, 50, dtype)
    image = im.Image(px.copy() if host else to_device(px))
    marked = np.full(px.shape, 12345, dtype=px.dtype)
    out = im.Image(marked if host else to_device(marked))
    lib = im.load()
    import ctypes
    limits = [(ADAPTIVE_MAX_WIDTH + 1, 3), (3, 65538)] if dtype == Q16 else \
        [(ADAPTIVE_FLOAT_MAX_SIDE + 1, 3), (3, ADAPTIVE_FLOAT_MAX_SIDE + 1)]
    for width, height in limits:
        status = lib.MagickHipAdaptiveThresholdImage(ctypes.byref(image.descriptor()), ctypes.byref(out.descriptor()),
                                                     width, height, 0.0)
        assert status == MH_UNSUPPORTED
        assert (out.numpy() == 12345).all(), "the destination was touched"
