"""The tables BilateralBlurImage and SelectiveBlurImage build on the host (kernel_info.cpp) against
the reference's expressions (effect.c:846-856, :951-970, :3456-3466) evaluated with this box's
libm through math.exp / math.sqrt: doubles, bit for bit.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

EPSILON = 1.0e-12
PI = 3.1415926535897932384626433832795028841971693993751058209749445923078164062
TWO_PI = 6.28318530717958647692528676655900576839433879875020


@pytest.fixture(scope="module")
def lib():
    import imagemagick_amd
    try:
        return imagemagick_amd.load()
    except Exception as error:                      # no HIP runtime on this box
        pytest.skip("libmagickhip.so does not load here: %s" % error)


def perceptible_reciprocal(x):
    sign = -1.0 if x < 0.0 else 1.0
    return 1.0 / x if sign * x >= EPSILON else sign / EPSILON


def blur_gaussian(x, sigma):
    return math.exp(-(x * x) * perceptible_reciprocal(2.0 * sigma * sigma)) * \
        perceptible_reciprocal(TWO_PI * sigma * sigma)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("width,height", [(1, 1), (3, 3), (5, 3), (1, 7), (9, 9), (15, 15), (33, 33), (0, 5)])
@pytest.mark.parametrize("sigmas", [(20.0, 3.0), (1.5, 0.8), (200.0, 10.0), (0.0, 0.0), (-2.0, 1e-13)])
def test_bilateral_tables(lib, width, height, sigmas):
    W, H = max(width, 1), max(height, 1)
    intensity = np.full(511, np.nan)
    spatial = np.full(W * H, np.nan)
    double_p = ctypes.POINTER(ctypes.c_double)
    assert lib.MhBilateralBlurTables(width, height, sigmas[0], sigmas[1], intensity.ctypes.data_as(double_p),
                                     spatial.ctypes.data_as(double_p)) == 0
    # entry 510 (a difference of +255) is never written by the reference; the library continues the series
    want = [blur_gaussian(float(w), sigmas[0]) for w in range(-255, 256)]
    assert same_bits(intensity, want)
    want = []
    for v in range(H):
        for u in range(W):
            du, dv = float(u - W // 2), float(v - H // 2)
            distance = math.sqrt((0.0 - du) * (0.0 - du) + (0.0 - dv) * (0.0 - dv))
            want.append(blur_gaussian(distance, sigmas[1]))
    assert same_bits(spatial, want)


@pytest.mark.parametrize("radius,sigma", [(0.0, 0.8), (0.0, 1.5), (0.0, 2.0), (3.0, 1.0), (0.0, 4.0), (2.0, 0.0),
                                          (1.0, -1.5)])
def test_selective_kernel(lib, radius, sigma):
    width = lib.MhSelectiveBlurKernel(radius, sigma, None)
    assert width == lib.MhGetOptimalKernelWidth1D(radius, sigma) and width % 2 == 1
    kernel = np.full(width * width, np.nan)
    assert lib.MhSelectiveBlurKernel(radius, sigma, kernel.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == width
    s = EPSILON if abs(sigma) < EPSILON else sigma          # MagickSigma, effect.c:132
    j = (width - 1) // 2
    want = [math.exp(-(float(u) * u + float(v * v)) / (2.0 * s * s)) / (2.0 * PI * s * s)
            for v in range(-j, j + 1) for u in range(-j, j + 1)]
    assert same_bits(kernel, want)
    assert kernel[(width * width) // 2] == kernel.max()      # not normalised: the centre is 1/(2 pi s^2)
