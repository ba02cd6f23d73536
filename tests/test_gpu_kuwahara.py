"""KuwaharaImage (effect.c:1775-1978) on the device against the compiled reference: Q16 and float
Quantum, 1-4 channels, both precision modes, host and device memory, every sample of every frame
bit-identical.  Within the documented window limit every call must succeed; only the two decline
tests accept MH_UNSUPPORTED."""
import ctypes

import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from kuwahara_oracle import (SHAPES, CHANNELS, cases, ref_kuwahara, plain4_reference, noise, sprite_alpha, constant,
                             flat_blocks, step_edge, wide_range_float, out_of_range_float)

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED = 1
RED, GREEN, BLUE, ALPHA = 0x1, 0x2, 0x4, 0x10                # ChannelType, pixel.h:49-78


def check(im, refmod, px, radius, sigma, what="", **settings):
    got = im.kuwahara_image(im.Image(to_device(px), **settings), radius, sigma).numpy()
    want = ref_kuwahara(refmod, refmod.RefImage(px), radius, sigma).numpy()
    assert_same(got, want, "kuwahara %gx%g %s %s %s" % (radius, sigma, px.shape, px.dtype.name, what))
    return got


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("index", range(len(SHAPES)))
def test_shapes_radii_sigmas_and_layouts(im, refmod, index, dtype):
    shape = SHAPES[index]
    for radius, sigma, layout in cases(index):
        px = noise(shape[0], shape[1], CHANNELS[layout], dtype)
        if layout == "plain4":
            got = im.kuwahara_image(im.Image(to_device(px), has_alpha=False), radius, sigma).numpy()
            assert_same(got, plain4_reference(refmod, px, radius, sigma), "plain 4-channel %s %g" % (shape, radius))
        else:
            check(im, refmod, px, radius, sigma, layout)


def test_the_case_list_covers_every_axis():
    seen = [set(), set(), set()]
    for index in range(len(SHAPES)):
        for case in cases(index):
            for axis, value in enumerate(case):
                seen[axis].add(value)
    assert [len(s) for s in seen] == [8, 3, 5]


# ------------------------------------------------------------------------------------------- alpha
@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_sprite_alpha(im, refmod, dtype, channels):
    """60 % of the alphas exactly 0: where all four fetched alphas are 0 the weight sum is below
    MagickEpsilon and PerceptibleReciprocal's clamp answers.  Even w: delta = 0, yet
    gamma*(alpha*p) is not always p."""
    px = sprite_alpha(noise(61, 97, channels, dtype))
    assert (px[..., -1] == 0).mean() > 0.5
    for radius in (1, 2, 3, 4):                               # w = 2, 3, 4, 5
        check(im, refmod, px, radius, 1.5, "sprite alpha")
    opaque = noise(45, 52, channels, dtype)
    opaque[..., -1] = 65535
    for radius in (1, 2):
        check(im, refmod, opaque, radius, 1.5, "alpha 65535 everywhere")


# ------------------------------------------------------------------------------------ channel masks
@pytest.mark.parametrize("mask,name,copied", [(RED, "R", (1, 2, 3)), (RED | GREEN | BLUE, "RGB", (3,)),
                                              (ALPHA, "A", (0, 1, 2))])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_channel_masks(im, refmod, dtype, mask, name, copied):
    """The channels outside the mask are copied by the blur and then interpolated like every other
    channel (in the plain form): they equal the reference's, not the source's."""
    px = sprite_alpha(noise(37, 52, 4, dtype), fraction=0.3)
    for radius in (1, 2):
        image = im.Image(to_device(px), channel_mask=mask, copy_channels=copied)
        got = im.kuwahara_image(image, radius, 1.5).numpy()
        want = ref_kuwahara(refmod, refmod.RefImage(px).set_channel_mask(name), radius, 1.5).numpy()
        assert_same(got, want, "channel mask %s" % name)
        for c in copied:
            assert (got[..., c] != px[..., c]).any(), "channel %d was passed through" % c


# -------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_ties(im, refmod, dtype, channels):
    for radius in (1, 2, 4):
        check(im, refmod, constant(40, 50, channels, dtype), radius, 1.5, "constant")
        check(im, refmod, flat_blocks(96, 128, channels, dtype), radius, 0.5, "flat blocks")
        check(im, refmod, step_edge(40, 50, channels, dtype), radius, 1.5, "step edge")


# ---------------------------------------------------------------------------------- float Quantum
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_float_ranges(im, refmod, channels):
    for radius in (1, 2, 3, 7):
        check(im, refmod, wide_range_float(61, 97, channels), radius, 1.5, "1e-3 ... 6e4")
        check(im, refmod, out_of_range_float(45, 52, channels), radius, 1.5, "negative and above QuantumRange")


# --------------------------------------------------------------------------------------- precision
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_both_precision_modes_give_the_reference(im, refmod, dtype):
    px = noise(61, 97, 4, dtype)
    for radius, sigma in [(2, 1.5), (3, 3)]:
        want = ref_kuwahara(refmod, refmod.RefImage(px), radius, sigma).numpy()
        for precision in (im.PRECISION_FAST, im.PRECISION_EXACT):
            got = im.kuwahara_image(im.Image(to_device(px), precision=precision), radius, sigma).numpy()
            assert_same(got, want, "MhImage.precision %d" % precision)
        im.set_precision(im.PRECISION_FAST)
        try:
            got = im.kuwahara_image(im.Image(to_device(px)), radius, sigma).numpy()
        finally:
            im.set_precision(im.PRECISION_EXACT)
        assert_same(got, want, "MhSetPrecision(FAST)")


def test_the_fast_blur_is_not_the_exact_one(im):
    """What the operator guards against: on this frame FAST BlurImage differs from EXACT somewhere, so
    an operator that passed the call's mode on to its blur would not get the reference's frame."""
    px = noise(61, 97, 4, Q16)
    differs = False
    for radius, sigma in [(2, 1.5), (3, 3)]:
        fast = im.blur_image(im.Image(to_device(px), precision=im.PRECISION_FAST), radius, sigma).numpy()
        exact = im.blur_image(im.Image(to_device(px), precision=im.PRECISION_EXACT), radius, sigma).numpy()
        assert np.abs(fast.astype(np.int64) - exact.astype(np.int64)).max() <= 1
        differs = differs or (fast != exact).any()
    assert differs, "FAST and EXACT BlurImage agree everywhere: the precision test above tests nothing"


# ------------------------------------------------------------------------------------------ memory
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_host_and_device_images(im, refmod, dtype):
    import torch
    px = noise(45, 70, 4, dtype)
    want = ref_kuwahara(refmod, refmod.RefImage(px), 2, 1.5).numpy()
    assert_same(im.kuwahara_image(im.Image(px.copy()), 2, 1.5).numpy(), want, "host image")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = to_device(px)
        got = im.kuwahara_image(im.Image(dev, stream=stream.cuda_stream), 2, 1.5)
    stream.synchronize()
    assert_same(got.numpy(), want, "device image on its own stream")


def test_through_the_c_abi_with_a_sentinel_behind_the_frame(im, refmod):
    """The descriptor filled by hand; the rows behind the frame keep their sentinel."""
    from imagemagick_amd import _lib
    lib = _lib.load()
    px = noise(33, 47, 4, Q16)
    src = to_device(px)
    dst = to_device(np.full((40, 47, 4), 0xABCD, dtype=np.uint16))
    a, b = _lib.MhImage(), _lib.MhImage()
    lib.MhInitImage(ctypes.byref(a), src.data_ptr(), 47, 33, 4, 1, _lib.QUANTUM_U16, _lib.MEMORY_DEVICE)
    lib.MhInitImage(ctypes.byref(b), dst.data_ptr(), 47, 33, 4, 1, _lib.QUANTUM_U16, _lib.MEMORY_DEVICE)
    a.device = b.device = 0
    assert lib.MagickHipKuwaharaImage(ctypes.byref(a), ctypes.byref(b), 3.0, 1.5) == 0
    import torch
    torch.cuda.synchronize()
    got = im.Image(dst).numpy()
    assert_same(got[:33], ref_kuwahara(refmod, refmod.RefImage(px), 3, 1.5).numpy(), "C ABI")
    assert (got[33:] == 0xABCD).all()


# ---------------------------------------------------------------------------------------- declines
def _declined_and_untouched(im, px, radius, sigma):
    sentinel = np.full(px.shape, 0x5A5A if px.dtype == np.uint16 else -77.0, dtype=px.dtype)
    from imagemagick_amd import _lib
    lib = _lib.load()
    for host in (False, True):
        src = im.Image(px.copy() if host else to_device(px))
        dst = im.Image(sentinel.copy() if host else to_device(sentinel))
        a, b = src.descriptor(), dst.descriptor()
        assert lib.MagickHipKuwaharaImage(ctypes.byref(a), ctypes.byref(b), radius, sigma) == MH_UNSUPPORTED
        assert np.array_equal(dst.numpy(), sentinel), "a declined call wrote to its destination"


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_radius_beyond_the_limit_is_declined(im, refmod, dtype):
    px = noise(20, 30, 4, dtype)
    _declined_and_untouched(im, px, 64.0, 1.5)
    _declined_and_untouched(im, px, 34.0 if dtype == Q16 else 27.0, 1.5)      # the first radius over the limit
    check(im, refmod, px, 33.0 if dtype == Q16 else 26.0, 1.5, "the last radius within the limit")


def test_what_the_blur_declines_is_declined(im):
    """A blur kernel whose row pass does not fit the LDS (float Quantum RGBA, 2815 taps):
    MagickHipBlurImage returns MH_UNSUPPORTED, and so does the operator that starts with it."""
    px = noise(20, 30, 4, HDRI)
    with pytest.raises(im.MagickHipError) as error:
        im.blur_image(im.Image(to_device(px), precision=im.PRECISION_EXACT), *BLUR_DECLINES)
    assert error.value.status == MH_UNSUPPORTED
    _declined_and_untouched(im, px, *BLUR_DECLINES)


BLUR_DECLINES = (0.0, 500.0)
