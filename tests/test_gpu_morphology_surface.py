"""Parts of MorphologyApply's generic surface no other test runs, bit-identical against the compiled reference in
EXACT mode on Q16 and float Quantum: Open/CloseIntensity, Erode/DilateIntensity on gray+alpha and on frames whose
colourspace or intensity method puts a gamma step into GetPixelIntensity, IterativeDistance under every distance
kernel, Correlate beside Convolve with asymmetric kernels on every layout, the generic methods on frames smaller
than their kernel, and the two methods the library declines.

Found with these tests, fixed in morphology.hip: Erode/DilateIntensity (and Open/CloseIntensity) of a linear-RGB
frame were declined ("intensity method needs a gamma transform") although the device restatement of
GetPixelIntensity the other operators use (pixel_intensity.hpp) is bit-exact; the generic kernel now calls it
where the method encodes or decodes the samples first."""
import ctypes

import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity
from edge_blur_oracle import set_intensity

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
ROWS, COLS = 45, 61
ASYMMETRIC = ["5x3+0+2: 0.1,0.2,-0.3,0.4,0.5 0,-0.1,0,0.1,0 -0.1,0.2,-0.1,0.2,-0.2",
              "3x5+2+4: 0.1,0.2,-0.3 0.4,0.5,0 0,-0.1,0.2 0.3,-0.2,0.1 0.05,0,0.15"]


def same(got, want, what):
    """Bit-identical; NaN where the reference has NaN (float frames)."""
    got = got.reshape(want.shape)
    if want.dtype == np.float32:
        equal = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert equal.all(), "%s: %d of %d float samples differ, first at %s" % (
            what, int((~equal).sum()), equal.size, np.argwhere(~equal)[:3].tolist())
    else:
        assert_parity(got, want, True, what)


def pair(im, refmod, px, colorspace="sRGB", intensity=None, **kw):
    ref = refmod.RefImage(px, colorspace)
    if intensity is not None:
        set_intensity(ref, intensity[0])
        kw["intensity"] = intensity[1]
    return im.Image(to_device(px), colorspace=colorspace.lower(), **kw), ref


DTYPES = pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
INTENSITY_FRAMES = {                                     # channels, colourspace, (-intensity method, its number)
    "graya": (2, "sRGB", None), "linear-rgb": (3, "RGB", None), "linear-rgba": (4, "RGB", None),
    "average": (3, "sRGB", ("Average", 1)), "linear-601luma": (3, "RGB", ("Rec601Luma", 5)),
    "709luminance": (3, "sRGB", ("Rec709Luminance", 8)), "601luminance-rgba": (4, "sRGB", ("Rec601Luminance", 6))}


@DTYPES
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_open_close_intensity(im, refmod, channels, dtype):
    for method in ("OpenIntensity", "CloseIntensity"):
        for kernel in ("Disk:2.5", "Rectangle:5x3+1+1"):
            for kind in ("random", "smooth"):
                px = make_pixels(ROWS, COLS, channels, dtype, seed=channels + len(kernel), kind=kind)
                dev, ref = pair(im, refmod, px)
                same(im.morphology_image(dev, method, 1, kernel).numpy(), ref.morphology(method, 1, kernel).numpy(),
                     "%s %s, %d channels, %s" % (method, kernel, channels, kind))


@DTYPES
@pytest.mark.parametrize("frame", list(INTENSITY_FRAMES))
def test_intensity_methods_read_the_colourspace_and_the_intensity_setting(im, refmod, frame, dtype):
    """GetPixelIntensity (pixel.c:2356-2455): gray+alpha weighs the gray sample three times; Rec601Luma / Rec709Luma
    of a linear-RGB frame encode the samples first, the Luminance methods of an sRGB frame decode them."""
    channels, colorspace, intensity = INTENSITY_FRAMES[frame]
    for method in ("ErodeIntensity", "DilateIntensity", "OpenIntensity"):
        for kernel in ("Disk:2.5", "Rectangle:5x3+1+1"):
            for kind in ("random", "smooth"):
                px = make_pixels(ROWS, COLS, channels, dtype, seed=channels + len(frame), kind=kind)
                dev, ref = pair(im, refmod, px, colorspace, intensity)
                same(im.morphology_image(dev, method, 1, kernel).numpy(), ref.morphology(method, 1, kernel).numpy(),
                     "%s %s, %s, %s" % (method, kernel, frame, kind))


@DTYPES
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_iterative_distance_kernels(im, refmod, channels, dtype):
    """On make_pixels' binary frames (no sample further than two steps from a black one) and on a frame of a few
    large white shapes, where the unbounded iteration runs a dozen passes before nothing changes."""
    for kernel in ("Manhattan:1", "Octagonal:1", "Euclidean:1", "Chebyshev:2"):
        speckle = make_pixels(ROWS, COLS, channels, dtype, seed=channels + len(kernel), kind="binary")
        shapes = np.zeros_like(speckle)
        shapes[3:30, 4:40] = 65535
        shapes[25:44, 35:60, : max(1, channels - 1)] = 65535
        shapes[10:14, 10:20] = 0
        for name, px in (("speckle", speckle), ("shapes", shapes)):
            dev, ref = pair(im, refmod, px)
            for iterations in (1, 3, -1):
                same(im.morphology_image(dev, "IterativeDistance", iterations, kernel).numpy(),
                     ref.morphology("IterativeDistance", iterations, kernel).numpy(),
                     "IterativeDistance %s x%d, %d channels, %s" % (kernel, iterations, channels, name))


@DTYPES
def test_correlate_and_convolve_asymmetric_kernels(im, refmod, dtype):
    """Correlate is Convolve with the kernel rotated by 180 degrees about its origin (morphology.c:3790): under a
    kernel that is no mirror image of itself, origin off centre, the two differ."""
    for layout, channels in (("gray", 1), ("graya", 2), ("rgb", 3), ("rgba", 4), ("plain4", 4)):
        for kernel in ASYMMETRIC:
            px = make_pixels(ROWS, COLS, channels, dtype, seed=channels + len(kernel))
            dev = im.Image(to_device(px), has_alpha=layout in ("graya", "rgba"))
            results = {}
            for method in ("Correlate", "Convolve"):
                if layout == "plain4":
                    want = np.concatenate([refmod.RefImage(px[:, :, c].copy()).morphology(method, 1, kernel).numpy()
                                           .reshape(ROWS, COLS, 1) for c in range(4)], axis=2)
                else:
                    want = refmod.RefImage(px).morphology(method, 1, kernel).numpy().reshape(px.shape)
                results[method] = im.morphology_image(dev, method, 1, kernel).numpy()
                same(results[method], want, "%s %s, %s" % (method, kernel[:8], layout))
            assert not np.array_equal(results["Correlate"], results["Convolve"]), (layout, kernel)


SMALL_FRAME_CASES = [("HitAndMiss", "Corners", 1), ("Thinning", "Skeleton", 2), ("Thicken", "ConvexHull", 1),
                     ("ErodeIntensity", "Disk:3", 1), ("IterativeDistance", "Chebyshev:1", 2), ("Edge", "Disk:2.5", 1),
                     ("TopHat", "Disk:2.5", 1), ("Smooth", "Disk:2.5", 1), ("Dilate", "Plus:1;Square:1", 1)]


@pytest.mark.parametrize("shape", [(1, 40), (40, 1), (2, 2), (3, 5)], ids=["1x40", "40x1", "2x2", "3x5"])
def test_generic_methods_on_frames_smaller_than_the_kernel(im, refmod, shape):
    for method, kernel, iterations in SMALL_FRAME_CASES:
        for kind in ("random", "binary"):
            px = make_pixels(shape[0], shape[1], 3, Q16, seed=shape[0] + len(kernel), kind=kind)
            dev, ref = pair(im, refmod, px)
            same(im.morphology_image(dev, method, iterations, kernel).numpy(),
                 ref.morphology(method, iterations, kernel).numpy(),
                 "%s %s x%d on %dx%d, %s" % (method, kernel, iterations, shape[0], shape[1], kind))


@DTYPES
@pytest.mark.parametrize("method,kernel", [("Distance", "Euclidean:1"), ("Voronoi", "Chebyshev:1")], ids=["distance", "voronoi"])
def test_declined_methods_leave_the_destination_alone(im, method, kernel, dtype):
    """Distance and Voronoi are sequential in the reference (MorphologyPrimitiveDirect) and declined: an error, and
    not one sample of the destination written."""
    px = make_pixels(ROWS, COLS, 3, dtype, kind="binary")
    sentinel = np.full(px.shape, 12345, dtype=dtype)
    dev, out = im.Image(to_device(px)), im.Image(to_device(sentinel.copy()))
    lib = im.load()
    with im._Kernel(kernel) as k:
        for iterations in (1, -1):
            with pytest.raises(im.MagickHipError):
                im._lib.check(lib.MagickHipMorphologyImage(ctypes.byref(dev.descriptor()), ctypes.byref(out.descriptor()),
                                                           im.MORPHOLOGY[method.lower()], iterations, k, 0.0))
            assert np.array_equal(out.numpy(), sentinel)
    with pytest.raises(im.MagickHipError):
        im.morphology_image(dev, method, 1, kernel)
    with pytest.raises(im.MagickHipError):
        im.morphology_primitive(dev, method, kernel)
