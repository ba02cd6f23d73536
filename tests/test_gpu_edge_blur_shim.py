"""BilateralBlurImage and SelectiveBlurImage through the HIP-backed MagickCore: the shim's hooks in
front of each operator's first CloneImage (effect.c) send the call to libmagickhip.so, and the
result is the pure-CPU one.  What the library does not serve - an even bilateral size, Tile
virtual pixels - is left to MagickCore's CPU code."""
import ctypes
import os

import numpy as np
import pytest

from conftest import make_pixels
from statistic_oracle import TILE_VIRTUAL_PIXELS, set_virtual_pixels, assert_same
from edge_blur_oracle import ref_bilateral, ref_selective, bilateral_pixels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(refmod, im):
    if not (os.path.exists(refmod.shim_lib_path(False)) and os.path.exists(refmod.shim_lib_path(True))):
        pytest.skip("the HIP-backed MagickCore (oracle/_ref/libMagickCore-hip-*.so) is not built")
    os.environ["MAGICK_HIP_LIBRARY"] = os.path.join(ROOT, "imagemagick_amd", "lib", "libmagickhip.so")
    return refmod


def has_edge_blur_hooks(refmod, hdri):
    """A HIP-backed MagickCore linked before these hooks existed resolves no
    MagickHipBilateralBlurImage (shim/opencl_hip.c) and runs both operators on the CPU."""
    with open(refmod.shim_lib_path(hdri), "rb") as f:
        data = f.read()
    return b"MagickHipBilateralBlurImage\0" in data and b"MagickHipSelectiveBlurImage\0" in data


def accelerated_calls(refmod, hdri):
    lib = refmod._load(hdri, True)
    lib.GetMagickHipAcceleratedCalls.restype = ctypes.c_size_t
    return lib.GetMagickHipAcceleratedCalls()


def need_hooks(shim, hdri):
    if not has_edge_blur_hooks(shim, hdri):
        pytest.skip("the HIP-backed MagickCore in oracle/_ref predates the edge-blur hooks (rebuild: make -C shim)")


@pytest.mark.parametrize("window,sigmas", [((3, 3), (20.0, 3.0)), ((9, 9), (20.0, 3.0)), ((5, 11), (200.0, 10.0))])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_bilateral_through_magickcore(shim, dtype, window, sigmas):
    hdri = dtype == np.float32
    need_hooks(shim, hdri)
    px = bilateral_pixels(70, 90, 4, dtype, seed=12)
    cpu = ref_bilateral(shim, shim.RefImage(px), window[0], window[1], *sigmas).numpy()
    before = accelerated_calls(shim, hdri)
    gpu = ref_bilateral(shim, shim.RefImage(px, shim=True), window[0], window[1], *sigmas).numpy()
    assert accelerated_calls(shim, hdri) == before + 1, "BilateralBlurImage did not take the accelerated path"
    assert_same(gpu, cpu, "BilateralBlurImage %s via MagickCore" % (window,))


@pytest.mark.parametrize("radius,sigma,threshold", [(0.0, 1.5, 6553.5), (3.0, 1.0, 655.35), (0.0, 2.0, 20000.0)])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_selective_through_magickcore(shim, dtype, channels, radius, sigma, threshold):
    hdri = dtype == np.float32
    need_hooks(shim, hdri)
    px = make_pixels(70, 90, channels, dtype, seed=13, kind="smooth")
    cpu = ref_selective(shim, shim.RefImage(px), radius, sigma, threshold).numpy()
    before = accelerated_calls(shim, hdri)
    gpu = ref_selective(shim, shim.RefImage(px, shim=True), radius, sigma, threshold).numpy()
    assert accelerated_calls(shim, hdri) == before + 1, "SelectiveBlurImage did not take the accelerated path"
    assert_same(gpu, cpu, "SelectiveBlurImage %gx%g+%g via MagickCore" % (radius, sigma, threshold))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_even_bilateral_size_is_left_to_the_cpu(shim, dtype):
    """An even side: the shim declines, the counter stays, MagickCore's own code answers.  What that
    code reads past its window is not defined, so its samples are not compared with another run's."""
    hdri = dtype == np.float32
    need_hooks(shim, hdri)
    px = bilateral_pixels(50, 64, 3, dtype, seed=14)
    before = accelerated_calls(shim, hdri)
    got = ref_bilateral(shim, shim.RefImage(px, shim=True), 4, 4, 20.0, 3.0).numpy()
    assert accelerated_calls(shim, hdri) == before, "an even bilateral size was accelerated"
    assert got.shape == px.shape and got.dtype == px.dtype
    # an odd size next to it is accelerated and equals the CPU result
    got = ref_bilateral(shim, shim.RefImage(px, shim=True), 5, 5, 20.0, 3.0).numpy()
    assert accelerated_calls(shim, hdri) == before + 1
    assert_same(got, ref_bilateral(shim, shim.RefImage(px), 5, 5, 20.0, 3.0).numpy(), "BilateralBlurImage 5x5")


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_tile_virtual_pixels_are_left_to_the_cpu(shim, dtype):
    hdri = dtype == np.float32
    need_hooks(shim, hdri)
    px = bilateral_pixels(50, 64, 3, dtype, seed=15)
    cpu = set_virtual_pixels(shim, shim.RefImage(px), TILE_VIRTUAL_PIXELS)
    gpu = set_virtual_pixels(shim, shim.RefImage(px, shim=True), TILE_VIRTUAL_PIXELS)
    before = accelerated_calls(shim, hdri)
    got = ref_bilateral(shim, gpu, 5, 5, 20.0, 3.0).numpy()
    assert_same(got, ref_bilateral(shim, cpu, 5, 5, 20.0, 3.0).numpy(), "BilateralBlurImage, Tile virtual pixels")
    got = ref_selective(shim, gpu, 0.0, 1.5, 6553.5).numpy()
    assert_same(got, ref_selective(shim, cpu, 0.0, 1.5, 6553.5).numpy(), "SelectiveBlurImage, Tile virtual pixels")
    assert accelerated_calls(shim, hdri) == before, "a Tile virtual-pixel call was accelerated"
