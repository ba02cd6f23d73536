"""MH_OP_THRESHOLD, MH_OP_AUTO_THRESHOLD and MH_OP_ADAPTIVE_THRESHOLD in MagickHipBatchImages: the same
bits as the direct calls.  MagickHipShardedImage declines all three."""
import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from threshold_oracle import noise

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
MH_UNSUPPORTED = 1
CHAINS = [[("threshold", 30000.25)], [("autothreshold", "Kapur")], [("autothreshold", "OTSU")],
          [("autothreshold", "Triangle")], [("adaptivethreshold", 7, 5, -655.35)],
          [("blur", 0.0, 1.0), ("adaptivethreshold", 25, 25, 1966.05)]]


def direct(im, px, chain):
    image = im.Image(to_device(px), precision=im.PRECISION_EXACT)
    for step in chain:
        if step[0] == "threshold":
            image = im.bilevel_image(image, step[1])
        elif step[0] == "autothreshold":
            image = im.auto_threshold_image(image, step[1])[0]
        elif step[0] == "adaptivethreshold":
            image = im.adaptive_threshold_image(image, *step[1:])
        else:
            image = im.blur_image(image, *step[1:])
    return image.numpy()


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("chain", CHAINS, ids=lambda chain: "+".join(step[0] for step in chain))
def test_batch_threshold_operators(im, chain, memory, dtype):
    pixels = [noise(48, 64, channels, dtype, seed=900 + channels) for channels in (1, 4, 3, 2)]
    for p in pixels:                 # images of a batch share the layout of their own result only
        image = im.Image(p.copy() if memory == "host" else to_device(p), precision=im.PRECISION_EXACT)
        result = image.like()
        report = im.batch_images(chain, [image], [result], devices=2, streams_per_device=2)
        assert sum(report["images_per_device"]) == 1
        assert_same(result.numpy(), direct(im, p, chain), "batch %s (%s, %d channels)" % (chain, memory, p.shape[2]))


def test_batch_of_several_images(im):
    pixels = [noise(48, 64, 4, Q16, seed=950 + i) for i in range(6)]
    chain = [("adaptivethreshold", 9, 9, 0.0)]
    images = [im.Image(to_device(p)) for p in pixels]
    results = [image.like() for image in images]
    report = im.batch_images(chain, images, results, devices=2, streams_per_device=2)
    assert report["devices"] == 2 and sum(report["images_per_device"]) == len(pixels)
    for p, result in zip(pixels, results):
        assert_same(result.numpy(), direct(im, p, chain), "batch of six")


@pytest.mark.parametrize("chain", CHAINS[:5], ids=lambda chain: chain[0][0])
def test_sharded_threshold_operators_are_declined(im, chain):
    px = noise(80, 96, 4, Q16, seed=61)
    with pytest.raises(im.MagickHipError) as error:
        im.sharded_image(chain, im.Image(px.copy()), devices=3)
    assert error.value.status == MH_UNSUPPORTED
