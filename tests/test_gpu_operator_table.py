"""Every MhOperatorKind through MagickHipBatchImages and MagickHipShardedImage, one one-operator chain each:
the batch layer describes a kind in one row of a table (batch.cpp), and this walks the table.  A batch equals
the direct call of the same library bit for bit; a sharded image does too, or the kind is one of those the
entry point declines.  The arguments and frames are those of each operator's own batch (or parity) test.

Frames of 50 rows x 40 columns: three bands are 16, 17 and 17 rows, so the cuts are unequal, both interior
cuts have a halo on either side, and every band is taller than the largest reach among the arguments."""
import ctypes

import numpy as np
import pytest

from conftest import make_pixels, to_device
from statistic_oracle import assert_same
from edge_blur_oracle import bilateral_pixels
from imagemagick_amd import _lib
import clahe_oracle
import kuwahara_oracle
import levels_oracle
import scale_oracle
import threshold_oracle

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED, MH_BAD_ARGUMENT = 1, 3
ROWS, COLUMNS, PIXELS = 50, 40, 50 * 40
TARGET = (23, 31)                                                  # columns x rows of the geometry-changing kinds


def random_rgba(dtype, seed):
    return make_pixels(ROWS, COLUMNS, 4, dtype, seed=seed)


def smooth_rgba(dtype, seed):                                      # ContrastStretch: a colour frame that is not gray
    return make_pixels(ROWS, COLUMNS, 4, dtype, seed=seed, kind="smooth")


def bilateral_rgba(dtype, seed):
    return bilateral_pixels(ROWS, COLUMNS, 4, dtype, seed=seed)


def clahe_rgba(dtype, seed):                                       # three colour channels, sRGB
    return clahe_oracle.noise(ROWS, COLUMNS, 4, dtype, seed=seed)


def kuwahara_rgba(dtype, seed):
    return kuwahara_oracle.noise(ROWS, COLUMNS, 4, dtype, seed=seed)


def threshold_rgba(dtype, seed):
    return threshold_oracle.noise(ROWS, COLUMNS, 4, dtype, seed=seed)


def levels_rgba(dtype, seed):
    return levels_oracle.frame("rgba", ROWS, COLUMNS, dtype, seed=seed)


def scale_rgba(dtype, seed):
    return scale_oracle.frame("rgba", ROWS, COLUMNS, dtype, seed=seed, transparent=0.2)


# kind -> (the chain's step, the frame, the direct call on a device image)
CASES = {
    "blur": (("blur", 0.0, 2.0), random_rgba, lambda im, x: im.blur_image(x, 0.0, 2.0)),
    "gaussianblur": (("gaussianblur", 0.0, 1.5), random_rgba, lambda im, x: im.gaussian_blur_image(x, 0.0, 1.5)),
    "unsharpmask": (("unsharpmask", 0.0, 2.0, 1.0, 0.02), random_rgba,
                    lambda im, x: im.unsharp_mask_image(x, 0.0, 2.0, 1.0, 0.02)),
    "resize": (("resize",) + TARGET + ("Lanczos",), random_rgba, lambda im, x: im.resize_image(x, *TARGET, "Lanczos")),
    "morphology": (("morphology", "Dilate", 1, "Disk:5"), random_rgba,
                   lambda im, x: im.morphology_image(x, "Dilate", 1, "Disk:5")),
    "colorspace": (("colorspace", "Lab"), random_rgba, lambda im, x: im.transform_image_colorspace(x, "Lab")),
    "contraststretch": (("contraststretch", 0.03 * PIXELS, PIXELS - 0.02 * PIXELS), smooth_rgba,
                        lambda im, x: im.contrast_stretch_image(x, 0.03 * PIXELS, PIXELS - 0.02 * PIXELS)),
    "equalize": (("equalize",), smooth_rgba, lambda im, x: im.equalize_image(x)),
    "statistic": (("statistic", "Median", 5, 5), random_rgba, lambda im, x: im.statistic_image(x, "Median", 5, 5)),
    "bilateralblur": (("bilateralblur", 5, 7, 20.0, 3.0), bilateral_rgba,
                      lambda im, x: im.bilateral_blur_image(x, 5, 7, 20.0, 3.0)),
    "selectiveblur": (("selectiveblur", 0.0, 1.5, 6553.5), bilateral_rgba,
                      lambda im, x: im.selective_blur_image(x, 0.0, 1.5, 6553.5)),
    "kuwahara": (("kuwahara", 2, 1.5), kuwahara_rgba, lambda im, x: im.kuwahara_image(x, 2, 1.5)),
    "clahe": (("clahe", 16, 16, 128, 2.0), clahe_rgba, lambda im, x: im.clahe_image(x, 16, 16, 128, 2.0)),
    "threshold": (("threshold", 30000.25), threshold_rgba, lambda im, x: im.bilevel_image(x, 30000.25)),
    "autothreshold": (("autothreshold", "OTSU"), threshold_rgba, lambda im, x: im.auto_threshold_image(x, "OTSU")[0]),
    "adaptivethreshold": (("adaptivethreshold", 7, 5, -655.35), threshold_rgba,
                          lambda im, x: im.adaptive_threshold_image(x, 7, 5, -655.35)),
    "level": (("level", 5000.0, 60000.0, 2.2), levels_rgba, lambda im, x: im.level_image(x, 5000.0, 60000.0, 2.2)),
    "levelize": (("levelize", 3000.0, 50000.0, 0.45), levels_rgba,
                 lambda im, x: im.levelize_image(x, 3000.0, 50000.0, 0.45)),
    "gamma": (("gamma", 2.2), levels_rgba, lambda im, x: im.gamma_image(x, 2.2)),
    "negate": (("negate", 0), levels_rgba, lambda im, x: im.negate_image(x, 0)),
    "sigmoidalcontrast": (("sigmoidalcontrast", 1, 5.0, 32767.5), levels_rgba,
                          lambda im, x: im.sigmoidal_contrast_image(x, 1, 5.0, 32767.5)),
    "autolevel": (("autolevel",), levels_rgba, lambda im, x: im.auto_level_image(x)),
    "linearstretch": (("linearstretch", 40.0, 20.0), levels_rgba,
                      lambda im, x: im.linear_stretch_image(x, 40.0, 20.0)[0]),
    "normalize": (("normalize",), levels_rgba, lambda im, x: im.normalize_image(x)),
    "sample": (("sample",) + TARGET, scale_rgba, lambda im, x: im.sample_image(x, *TARGET)),
    "scale": (("scale",) + TARGET, scale_rgba, lambda im, x: im.scale_image(x, *TARGET)),
    "thumbnail": (("thumbnail",) + TARGET, scale_rgba, lambda im, x: im.thumbnail_image(x, *TARGET)),
}
CHANGE_GEOMETRY = {"resize", "sample", "scale", "thumbnail"}
# what MagickHipShardedImage declines, written out: the table's last column must say the same
DECLINED = {"resize", "sample", "scale", "thumbnail", "clahe", "threshold", "autothreshold", "adaptivethreshold",
            "autolevel", "linearstretch", "normalize"}


def test_every_kind_has_a_case():
    assert set(CASES) == set(_lib.OPERATORS)
    assert all(step[0] == kind for kind, (step, _, _) in CASES.items())


# over the binding's own list: a kind without a case fails here, it is not left out
@pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "hdri"])
@pytest.mark.parametrize("kind", sorted(_lib.OPERATORS, key=_lib.OPERATORS.get))
def test_batch_and_shards_equal_the_direct_call(im, kind, dtype):
    step, frame, call = CASES[kind]
    pixels = [frame(dtype, 40 + i) for i in range(3)]
    direct = [call(im, im.Image(to_device(p), precision=im.PRECISION_EXACT)).numpy() for p in pixels]

    images = [im.Image(p.copy(), precision=im.PRECISION_EXACT) for p in pixels]
    if kind in CHANGE_GEOMETRY:
        with pytest.raises(im.MagickHipError) as error:
            im.batch_images([step], images, None, devices=2, streams_per_device=1)
        assert error.value.status == MH_BAD_ARGUMENT
        results = [image.like(rows=TARGET[1], columns=TARGET[0]) for image in images]
    else:
        results = [image.like() for image in images]
    report = im.batch_images([step], images, results, devices=2, streams_per_device=1)
    assert report["devices"] == 2 and sum(report["images_per_device"]) == 3
    for k, (p, image, result, want) in enumerate(zip(pixels, images, results, direct)):
        assert np.array_equal(image.numpy(), p), "batch %s changed its input %d" % (kind, k)
        assert_same(result.numpy(), want, "batch %s, image %d" % (kind, k))

    image = im.Image(pixels[0].copy(), precision=im.PRECISION_EXACT)
    if kind in DECLINED:
        with pytest.raises(im.MagickHipError) as error:
            im.sharded_image([step], image, devices=3)
        assert error.value.status == MH_UNSUPPORTED
    else:
        result, report = im.sharded_image([step], image, devices=3)
        assert report["devices"] == 3 and report["halo_exchanges"] == 0
        assert_same(result.numpy(), direct[0], "sharded %s, 3 bands" % kind)


def test_sharded_morphology_until_convergence_is_declined(im):
    image = im.Image(random_rgba(Q16, 40))
    with pytest.raises(im.MagickHipError) as error:
        im.sharded_image([("morphology", "Dilate", -1, "Disk:5")], image, devices=3)
    assert error.value.status == MH_UNSUPPORTED


@pytest.mark.parametrize("kind", [0, max(_lib.OPERATORS.values()) + 1])
def test_a_kind_outside_the_table_is_a_bad_argument(im, kind):
    lib = im.load()
    op = _lib.MhOperator()
    op.kind = kind
    px = random_rgba(Q16, 40)
    image, result = im.Image(px.copy()), im.Image(np.full_like(px, 77))
    src, dst = image.descriptor(), result.descriptor()
    report = _lib.MhBatchReport()
    status = lib.MagickHipBatchImages(ctypes.byref(op), 1, ctypes.byref(src), ctypes.byref(dst), 1, 2, 1,
                                      ctypes.byref(report))
    assert status == MH_BAD_ARGUMENT and b"unknown kind %d" % kind in lib.MhGetLastError()
    status = lib.MagickHipShardedImage(ctypes.byref(op), 1, ctypes.byref(src), ctypes.byref(dst), 3,
                                       ctypes.byref(report))
    assert status == MH_BAD_ARGUMENT and b"unknown kind %d" % kind in lib.MhGetLastError()
    assert np.array_equal(image.numpy(), px) and np.array_equal(result.numpy(), np.full_like(px, 77))
