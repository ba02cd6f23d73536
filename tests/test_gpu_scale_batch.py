"""MH_OP_SAMPLE, MH_OP_SCALE and MH_OP_THUMBNAIL in MagickHipBatchImages: a batch of mixed-size images
equals the per-image calls; like MH_OP_RESIZE they change the geometry, so a chain that holds one needs
result descriptors, and MagickHipShardedImage declines all three."""
import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from scale_oracle import frame

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED, MH_BAD_ARGUMENT = 1, 3
SIZES = [(120, 90), (97, 61), (200, 150), (64, 64), (333, 131), (48, 100), (150, 201), (80, 80)]     # rows x columns
TARGET = (24, 20)                                                                                      # rows x columns


def batch(im, dtype, memory):
    pixels = [frame("rgba", rows, cols, dtype, seed=700 + k, transparent=0.2) for k, (rows, cols) in enumerate(SIZES)]
    images = [im.Image(p.copy() if memory == "host" else to_device(p), precision=im.PRECISION_EXACT) for p in pixels]
    return pixels, images


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_a_batch_of_thumbnails_equals_the_calls_one_by_one(im, memory, dtype):
    pixels, images = batch(im, dtype, memory)
    results = [image.like(rows=TARGET[0], columns=TARGET[1]) for image in images]
    report = im.batch_images([("thumbnail", TARGET[1], TARGET[0])], images, results, devices=2, streams_per_device=2)
    assert sum(report["images_per_device"]) == len(images)
    for k, (p, result) in enumerate(zip(pixels, results)):
        direct = im.thumbnail_image(im.Image(to_device(p), precision=im.PRECISION_EXACT), TARGET[1], TARGET[0])
        assert_same(result.numpy(), direct.numpy(), "thumbnail of image %d (%s)" % (k, memory))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("first", ["scale", "sample"])
def test_a_chain_behind_a_scale_equals_the_calls_one_by_one(im, first, memory, dtype):
    pixels, images = batch(im, dtype, memory)
    results = [image.like(rows=TARGET[0], columns=TARGET[1]) for image in images]
    im.batch_images([(first, TARGET[1], TARGET[0]), ("blur", 0, 1.5)], images, results, devices=2, streams_per_device=2)
    call = im.scale_image if first == "scale" else im.sample_image
    for k, (p, result) in enumerate(zip(pixels, results)):
        direct = im.blur_image(call(im.Image(to_device(p), precision=im.PRECISION_EXACT), TARGET[1], TARGET[0]), 0, 1.5)
        assert_same(result.numpy(), direct.numpy(), "%s + blur of image %d (%s)" % (first, k, memory))


@pytest.mark.parametrize("chain", [[("sample", 20, 24)], [("scale", 20, 24)], [("thumbnail", 20, 24)],
                                   [("negate", 0), ("scale", 20, 24)]], ids=lambda chain: chain[-1][0])
def test_a_chain_without_result_descriptors_is_a_bad_argument(im, chain):
    px = frame("rgba", 48, 64, Q16, seed=1)
    image = im.Image(to_device(px))
    with pytest.raises(im.MagickHipError) as error:
        im.batch_images(chain, [image])
    assert error.value.status == MH_BAD_ARGUMENT
    assert np.array_equal(image.numpy(), px)


@pytest.mark.parametrize("chain", [[("sample", 64, 48)], [("scale", 64, 48)], [("thumbnail", 64, 48)]],
                         ids=lambda chain: chain[-1][0])
def test_a_sharded_request_is_declined_untouched(im, chain):
    px = frame("rgba", 48, 64, Q16, seed=2)
    image, result = im.Image(px.copy()), im.Image(np.full_like(px, 77))
    with pytest.raises(im.MagickHipError) as error:
        im.sharded_image(chain, image, result, devices=2)
    assert error.value.status == MH_UNSUPPORTED
    assert np.array_equal(image.numpy(), px) and np.array_equal(result.numpy(), np.full_like(px, 77))
