"""MH_OP_CLAHE in MagickHipBatchImages: the same bits as one call of the operator and as the
compiled reference.  MagickHipShardedImage declines it: the tile grid belongs to the whole frame."""
import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from clahe_oracle import noise, reference

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED = 1


@pytest.mark.parametrize("memory", ["host", "device"])
def test_batch_clahe(im, refmod, memory):
    pixels = [noise(48, 64, 4, Q16, seed=700 + i) for i in range(6)]
    chain = [("clahe", 16, 16, 128, 2.0)]
    images = [im.Image(p.copy() if memory == "host" else to_device(p)) for p in pixels]
    results = [image.like() for image in images]
    report = im.batch_images(chain, images, results, devices=2, streams_per_device=2)
    assert report["devices"] == 2 and sum(report["images_per_device"]) == len(pixels)
    for p, result in zip(pixels, results):
        one = im.clahe_image(im.Image(to_device(p)), 16, 16, 128, 2.0).numpy()
        assert_same(result.numpy(), one, "batch clahe (%s)" % memory)
        assert_same(one, reference(refmod, p, "sRGB", 16, 16, 128, 2.0), "single clahe")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_batch_blur_then_clahe(im, dtype):
    pixels = [noise(48, 64, 4, dtype, seed=800 + i) for i in range(4)]
    chain = [("blur", 0.0, 1.0), ("clahe", 0, 0, 0, 3.0)]
    images = [im.Image(to_device(p), precision=im.PRECISION_EXACT) for p in pixels]
    results = [image.like() for image in images]
    im.batch_images(chain, images, results, devices=2, streams_per_device=2)
    for p, result in zip(pixels, results):
        blurred = im.blur_image(im.Image(to_device(p), precision=im.PRECISION_EXACT), 0.0, 1.0)
        one = im.clahe_image(blurred, 0, 0, 0, 3.0).numpy()
        assert_same(result.numpy(), one, "batch blur + clahe")


def test_sharded_clahe_is_declined(im):
    px = noise(80, 96, 4, Q16, seed=61)
    with pytest.raises(im.MagickHipError) as error:
        im.sharded_image([("clahe", 16, 16, 128, 2.0)], im.Image(px.copy()), devices=3)
    assert error.value.status == MH_UNSUPPORTED
