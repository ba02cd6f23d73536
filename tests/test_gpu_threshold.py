"""BilevelImage, AutoThresholdImage, BlackThresholdImage, WhiteThresholdImage and RangeThresholdImage
(MagickCore/threshold.c) on the device against the compiled reference: every sample equal, Q16 and
float Quantum, every layout, host and device memory, both precision modes."""
import ctypes

import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from threshold_oracle import (kept_channels_equal, SHAPES, LAYOUTS, CHANNELS, METHODS, INTENSITIES, MASKS, QR, ref_image, ref_bilevel,
                              ref_auto_threshold, ref_black_threshold, ref_white_threshold, ref_range_threshold, frame,
                              two_level, constant, out_of_range_float)

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED = 1
RANGES = [(10000.0, 20000.0, 40000.0, 50000.0), (15000.5, 15000.5, 30000.0, 61000.25), (0.0, 0.0, QR, QR),
          (20000.0, 20000.0 + 1.0e-13, 40000.0, 40000.0), (-5000.0, 100.0, 70000.0, 80000.0)]


def device_image(im, px, layout="rgba", host=False, **kw):
    return im.Image(px.copy() if host else to_device(px), has_alpha=layout in ("gray+alpha", "rgba"), **kw)


def thresholds_of(px):
    """0, QuantumRange, a sample of the frame (the <= / < tie) and a fractional value."""
    r, c = px.shape[0] // 2, px.shape[1] // 2
    return [0.0, QR, float(px[r, c, 0]), 30000.25]


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bilevel_and_auto(im, refmod, shape, layout, dtype):
    px = frame(layout, shape[0], shape[1], dtype)
    what = "%s %s %s" % (shape, layout, px.dtype.name)
    for threshold in thresholds_of(px):
        got = im.bilevel_image(device_image(im, px, layout), threshold).numpy()
        assert_same(got, ref_bilevel(ref_image(refmod, px), threshold).numpy(), "bilevel %g %s" % (threshold, what))
    for method in METHODS:
        image, percent = im.auto_threshold_image(device_image(im, px, layout), method)
        want, text = ref_auto_threshold(ref_image(refmod, px), method)
        assert "%g%%" % percent == text, "auto %s %s" % (method, what)
        assert_same(image.numpy(), want.numpy(), "auto %s %s" % (method, what))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", ["rgb", "rgba", "plain4"])
@pytest.mark.parametrize("shape", SHAPES)
def test_black_white_range(im, refmod, shape, layout, dtype):
    px = frame(layout, shape[0], shape[1], dtype, seed=3)
    what = "%s %s %s" % (shape, layout, px.dtype.name)
    channels = px.shape[2]
    for tie in thresholds_of(px):
        thresholds = [tie, 20000.5, 41000.0, 30000.0][:channels]
        got = im.black_threshold_image(device_image(im, px, layout), thresholds).numpy()
        assert_same(got, ref_black_threshold(ref_image(refmod, px), thresholds).numpy(), "black %s %s" % (thresholds, what))
        got = im.white_threshold_image(device_image(im, px, layout), thresholds).numpy()
        assert_same(got, ref_white_threshold(ref_image(refmod, px), thresholds).numpy(), "white %s %s" % (thresholds, what))
    r, c = px.shape[0] // 2, px.shape[1] // 2
    for points in RANGES + [(float(px[0, 0, 0]), float(px[r, c, 1]), float(px[r, c, 1]), 64000.0)]:
        got = im.range_threshold_image(device_image(im, px, layout), *points).numpy()
        assert_same(got, ref_range_threshold(ref_image(refmod, px), *points).numpy(), "range %s %s" % (points, what))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask", list(MASKS))
def test_channel_masks(im, refmod, mask, dtype):
    """With a channel mask every channel is decided by its own sample; channels outside it keep the source."""
    bits, copied = MASKS[mask]
    px = frame("rgba", 61, 97, dtype, seed=5)
    kept = list(copied)
    tie = float(px[30, 40, 0 if mask != "A" else 3])
    thresholds = [tie, 20000.5, 41000.0, 30000.0]

    def image():
        return device_image(im, px, channel_mask=bits, copy_channels=copied)

    results = [
        ("bilevel", im.bilevel_image(image(), tie), ref_bilevel(ref_image(refmod, px, mask=mask), tie)),
        ("black", im.black_threshold_image(image(), thresholds), ref_black_threshold(ref_image(refmod, px, mask=mask), thresholds)),
        ("white", im.white_threshold_image(image(), thresholds), ref_white_threshold(ref_image(refmod, px, mask=mask), thresholds)),
        ("range", im.range_threshold_image(image(), *RANGES[0]), ref_range_threshold(ref_image(refmod, px, mask=mask), *RANGES[0])),
        ("auto", im.auto_threshold_image(image(), "OTSU")[0], ref_auto_threshold(ref_image(refmod, px, mask=mask), "OTSU")[0]),
    ]
    for name, got, want in results:
        got = got.numpy()
        assert_same(got, want.numpy(), "%s mask %s %s" % (name, mask, px.dtype.name))
        assert kept_channels_equal(got, px, kept), "%s: untouched channels" % name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_float_samples_outside_the_quantum_range(im, refmod, layout):
    px = out_of_range_float(61, 97, CHANNELS[layout])
    for threshold in (-100.5, 0.0, 30000.25, QR, 70000.0):
        got = im.bilevel_image(device_image(im, px, layout), threshold).numpy()
        assert_same(got, ref_bilevel(ref_image(refmod, px), threshold).numpy(), "bilevel %g %s" % (threshold, layout))
    for method in METHODS:
        image, percent = im.auto_threshold_image(device_image(im, px, layout), method)
        want, text = ref_auto_threshold(ref_image(refmod, px), method)
        assert "%g%%" % percent == text
        assert_same(image.numpy(), want.numpy(), "auto %s %s" % (method, layout))
    if CHANNELS[layout] >= 3:
        for points in RANGES:
            got = im.range_threshold_image(device_image(im, px, layout), *points).numpy()
            assert_same(got, ref_range_threshold(ref_image(refmod, px), *points).numpy(), "range %s %s" % (points, layout))
        thresholds = [-50.0, 20000.5, 66000.0, 30000.0][:CHANNELS[layout]]
        got = im.black_threshold_image(device_image(im, px, layout), thresholds).numpy()
        assert_same(got, ref_black_threshold(ref_image(refmod, px), thresholds).numpy(), "black %s" % layout)
        got = im.white_threshold_image(device_image(im, px, layout), thresholds).numpy()
        assert_same(got, ref_white_threshold(ref_image(refmod, px), thresholds).numpy(), "white %s" % layout)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("colorspace", ["sRGB", "RGB"])
@pytest.mark.parametrize("method", list(INTENSITIES))
def test_intensity_methods(im, refmod, method, colorspace, dtype):
    """Every MhIntensityMethod, on an sRGB and a linear-RGB frame; BilevelImage retags the frame sRGB
    before it forms the intensity, AutoThresholdImage's counts see the colourspace as it was."""
    px = frame("rgba", 61, 97, dtype, seed=7)
    image = device_image(im, px, colorspace=colorspace, intensity=INTENSITIES[method])
    got = im.bilevel_image(image, 28000.5)
    assert image.colorspace == "srgb"
    want = ref_bilevel(ref_image(refmod, px, colorspace, intensity=method), 28000.5)
    assert_same(got.numpy(), want.numpy(), "bilevel %s %s" % (method, colorspace))
    image = device_image(im, px, colorspace=colorspace, intensity=INTENSITIES[method])
    got, percent = im.auto_threshold_image(image, "OTSU")
    want, text = ref_auto_threshold(ref_image(refmod, px, colorspace, intensity=method), "OTSU")
    assert "%g%%" % percent == text, (method, colorspace)
    assert_same(got.numpy(), want.numpy(), "auto %s %s" % (method, colorspace))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", ["gray", "rgba"])
def test_auto_threshold_constant_and_two_level(im, refmod, layout, dtype):
    for what, px in (("constant", constant(61, 97, CHANNELS[layout], dtype)),
                     ("two levels", two_level(61, 97, CHANNELS[layout], dtype))):
        for method in METHODS:
            image, percent = im.auto_threshold_image(device_image(im, px, layout), method)
            want, text = ref_auto_threshold(ref_image(refmod, px), method)
            assert "%g%%" % percent == text, "%s %s %s" % (what, method, layout)
            assert_same(image.numpy(), want.numpy(), "auto %s %s %s" % (what, method, layout))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("host", [False, True])
def test_memory_kinds_and_precision_modes(im, refmod, host, dtype):
    """Host and device memory; both MhSetPrecision modes give the same bits."""
    px = frame("rgba", 61, 97, dtype, seed=9)
    tie = float(px[10, 10, 0])
    want = {"bilevel": ref_bilevel(ref_image(refmod, px), tie).numpy(),
            "auto": ref_auto_threshold(ref_image(refmod, px), "Kapur")[0].numpy(),
            "black": ref_black_threshold(ref_image(refmod, px), [tie] * 4).numpy(),
            "white": ref_white_threshold(ref_image(refmod, px), [tie] * 4).numpy(),
            "range": ref_range_threshold(ref_image(refmod, px), *RANGES[0]).numpy()}
    try:
        for precision in (im.PRECISION_FAST, im.PRECISION_EXACT):
            im.set_precision(precision)
            got = {"bilevel": im.bilevel_image(device_image(im, px, host=host), tie),
                   "auto": im.auto_threshold_image(device_image(im, px, host=host), "Kapur")[0],
                   "black": im.black_threshold_image(device_image(im, px, host=host), tie),
                   "white": im.white_threshold_image(device_image(im, px, host=host), tie),
                   "range": im.range_threshold_image(device_image(im, px, host=host), *RANGES[0])}
            for name in want:
                assert_same(got[name].numpy(), want[name], "%s host=%s precision %d" % (name, host, precision))
    finally:
        im.set_precision(im.PRECISION_EXACT)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout,colorspace", [("gray", "srgb"), ("gray+alpha", "srgb"), ("rgb", "gray"), ("rgba", "lineargray")])
def test_gray_frames_are_declined_untouched(im, layout, colorspace, dtype):
    """Black, White and Range re-lay a gray frame out as sRGB in the reference: MH_UNSUPPORTED."""
    px = frame(layout, 15, 17, dtype)
    calls = [lambda image: im.black_threshold_image(image, 30000.0), lambda image: im.white_threshold_image(image, 30000.0),
             lambda image: im.range_threshold_image(image, *RANGES[0])]
    for host in (False, True):
        for call in calls:
            image = device_image(im, px, layout, host=host, colorspace=colorspace)
            with pytest.raises(im.MagickHipError) as error:
                call(image)
            assert error.value.status == MH_UNSUPPORTED
            assert np.array_equal(image.numpy().view(np.uint8), px.view(np.uint8))
