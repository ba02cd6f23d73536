"""CLAHEImage (enhance.c:295-785) on the device against the compiled reference.  The core (frames
declared Lab: no conversion runs) is bit-identical on Q16 and float Quantum; the whole operator is
bit-identical on Q16 in both precision modes (the call pins its conversions to the exact ones); on
float Quantum from sRGB the call equals the device's own transform -> core -> transform chain, and
the core on that device-made Lab frame equals the reference's."""
import ctypes

import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from clahe_oracle import (SHAPES, INPUTS, cases, reference, noise, constant, float_specials)

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED, MH_BAD_ARGUMENT = 1, 3


def core(im, refmod, px, width, height, number_bins, clip_limit, what="", key=None):
    got = im.clahe_image(im.Image(to_device(px), colorspace="Lab"), width, height, number_bins, clip_limit).numpy()
    want = reference(refmod, px, "Lab", width, height, number_bins, clip_limit, key=key)
    assert_same(got, want, "clahe %dx%d bins %d clip %g %s %s %s" % (width, height, number_bins, clip_limit, px.shape,
                                                                     px.dtype.name, what))
    return got


# ------------------------------------------------------------------------------------------- core
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("index", range(len(SHAPES)))
def test_core_shapes_bins_and_clip_limits(im, refmod, index, dtype):
    rows, cols, width, height = SHAPES[index]
    for number_bins, clip_limit, channels in cases(index):
        px = noise(rows, cols, channels, dtype)
        got = core(im, refmod, px, width, height, number_bins, clip_limit, key="noise")
        assert np.array_equal(got[..., 1:], px[..., 1:]), "a channel other than L was written"


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_core_structured_inputs(im, refmod, name, dtype):
    for (rows, cols, width, height), number_bins, clip_limit in [((61, 97, 16, 16), 128, 2.0), ((33, 50, 7, 5), 3, 1.5),
                                                                 ((64, 64, 8, 8), 255, 0.5)]:
        core(im, refmod, INPUTS[name](rows, cols, 4, dtype), width, height, number_bins, clip_limit, name, key=name)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_core_constant_frame_with_several_workgroups_a_tile(im, refmod, dtype):
    """Everything in one bin of 256 x 128 tiles: every lane of every wave counts the same bin, the
    clip leaves more excess than bins (whole sweeps) and then a strided remainder."""
    core(im, refmod, constant(1030, 2051, 4, dtype), 0, 0, 128, 2.0, "constant", key="constant big")


def test_core_float_specials(im, refmod):
    for (rows, cols, width, height), number_bins, clip_limit in [((61, 97, 16, 16), 128, 2.0), ((33, 50, 7, 5), 3, 1.0)]:
        core(im, refmod, float_specials(rows, cols, 3), width, height, number_bins, clip_limit, "float specials",
             key="specials")


def test_core_ignores_the_channel_mask(im, refmod):
    """The reference writes L back past the mask and the traits (enhance.c:761)."""
    px = noise(61, 97, 4, Q16)
    image = im.Image(to_device(px), colorspace="Lab", channel_mask=0x2, copy_channels=(0, 2, 3))     # GreenChannel, pixel.h:49-78
    got = im.clahe_image(image, 16, 16, 128, 2.0).numpy()
    want = reference(refmod, px, "Lab", 16, 16, 128, 2.0, key="noise")
    assert_same(got, want, "channel mask G")


# --------------------------------------------------------------------------------- whole operator
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("channels", [3, 4])
def test_whole_operator_srgb_q16_in_both_precision_modes(im, refmod, channels, memory):
    px = noise(61, 97, channels, Q16)
    for width, height, number_bins, clip_limit in [(16, 16, 128, 2.0), (0, 0, 0, 4.0), (16, 16, 128, 1.0)]:
        want = reference(refmod, px, "sRGB", width, height, number_bins, clip_limit, key="srgb")
        for precision in (im.PRECISION_FAST, im.PRECISION_EXACT):
            image = im.Image(px.copy() if memory == "host" else to_device(px), precision=precision)
            got = im.clahe_image(image, width, height, number_bins, clip_limit)
            assert got.colorspace == "srgb"
            assert_same(got.numpy(), want, "sRGB %s MhImage.precision %d clip %g" % (memory, precision, clip_limit))
        im.set_precision(im.PRECISION_FAST)
        try:
            got = im.clahe_image(im.Image(px.copy() if memory == "host" else to_device(px)), width, height,
                                 number_bins, clip_limit).numpy()
        finally:
            im.set_precision(im.PRECISION_EXACT)
        assert_same(got, want, "sRGB %s MhSetPrecision(FAST) clip %g" % (memory, clip_limit))


def test_clip_limit_one_is_the_lab_round_trip(im, refmod):
    px = noise(61, 97, 4, Q16)
    got = im.clahe_image(im.Image(to_device(px)), 16, 16, 128, 1.0).numpy()
    trip = im.Image(to_device(px), precision=im.PRECISION_EXACT)
    im.transform_image_colorspace(trip, "Lab")
    im.transform_image_colorspace(trip, "sRGB")
    assert_same(got, trip.numpy(), "clip_limit 1.0")
    assert (got != px).any(), "the round trip through Lab is the identity: the case tests nothing"


def test_the_fast_conversion_is_not_the_exact_one(im):
    """What the call guards against: FAST sRGB -> Lab differs from EXACT somewhere on this frame."""
    px = noise(61, 97, 4, Q16)
    fast = im.transform_image_colorspace(im.Image(to_device(px), precision=im.PRECISION_FAST), "Lab").numpy()
    exact = im.transform_image_colorspace(im.Image(to_device(px), precision=im.PRECISION_EXACT), "Lab").numpy()
    assert (fast != exact).any(), "FAST and EXACT sRGB -> Lab agree everywhere: the precision tests test nothing"


def test_hsl_source_returns_to_hsl(im, refmod):
    px = noise(61, 97, 4, Q16)
    want = reference(refmod, px, "HSL", 16, 16, 128, 2.0, key="hsl")
    image = im.Image(to_device(px), colorspace="HSL")
    got = im.clahe_image(image, 16, 16, 128, 2.0)
    assert got.colorspace == "hsl"
    assert_same(got.numpy(), want, "HSL source")


# ---------------------------------------------------------------------------- float Quantum, sRGB
@pytest.mark.parametrize("channels", [3, 4])
def test_float_srgb_is_the_device_chain_and_its_core_is_the_reference(im, refmod, channels):
    px = noise(61, 97, channels, HDRI)
    for width, height, number_bins, clip_limit in [(16, 16, 128, 2.0), (0, 0, 0, 4.0)]:
        got = im.clahe_image(im.Image(to_device(px)), width, height, number_bins, clip_limit).numpy()
        lab = im.Image(to_device(px), precision=im.PRECISION_EXACT)
        im.transform_image_colorspace(lab, "Lab")
        lab_px = lab.numpy().copy()
        im.clahe_image(lab, width, height, number_bins, clip_limit)
        core_px = lab.numpy().copy()
        im.transform_image_colorspace(lab, "sRGB")
        assert_same(got, lab.numpy(), "float sRGB against the device's own chain")
        assert_same(core_px, reference(refmod, lab_px, "Lab", width, height, number_bins, clip_limit),
                    "the core on the device-made Lab frame")


# ---------------------------------------------------------------------------------------- declines
def _declined_and_untouched(im, px, status, width, height, number_bins, clip_limit, **settings):
    from imagemagick_amd import _lib
    lib = _lib.load()
    for host in (False, True):
        image = im.Image(px.copy() if host else to_device(px), **settings)
        d = image.descriptor()
        assert lib.MagickHipCLAHEImage(ctypes.byref(d), width, height, number_bins, clip_limit) == status
        assert np.array_equal(image.numpy(), px), "a declined call wrote to the image"


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_layouts_the_reference_relays_are_declined(im, dtype):
    _declined_and_untouched(im, noise(40, 48, 1, dtype), MH_UNSUPPORTED, 8, 8, 128, 2.0, colorspace="Gray")
    _declined_and_untouched(im, noise(40, 48, 2, dtype), MH_UNSUPPORTED, 8, 8, 128, 2.0, colorspace="Gray")
    _declined_and_untouched(im, noise(40, 48, 4, dtype), MH_UNSUPPORTED, 8, 8, 128, 2.0, has_alpha=False)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_divisions_by_zero_are_bad_arguments(im, dtype):
    _declined_and_untouched(im, noise(40, 7, 4, dtype), MH_BAD_ARGUMENT, 0, 8, 128, 2.0)
    _declined_and_untouched(im, noise(7, 40, 4, dtype), MH_BAD_ARGUMENT, 8, 0, 128, 2.0)
    _declined_and_untouched(im, noise(40, 48, 4, dtype), MH_BAD_ARGUMENT, 8, 8, 1, 2.0)


def test_tile_maps_larger_than_the_frame_are_declined(im):
    # 1600 tiles x 128 bins x 2 bytes against 40 x 40 x 4 x 2
    _declined_and_untouched(im, noise(40, 40, 4, Q16), MH_UNSUPPORTED, 1, 1, 128, 2.0)


def test_a_colourspace_without_a_device_transform_is_declined(im):
    _declined_and_untouched(im, noise(40, 48, 4, Q16), MH_UNSUPPORTED, 8, 8, 128, 2.0, colorspace="LinearGray")
