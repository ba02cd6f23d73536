"""MH_OP_BILATERAL_BLUR and MH_OP_SELECTIVE_BLUR in MagickHipBatchImages and MagickHipShardedImage:
the same bits as one call of the operator.  A bilateral blur reaches H/2 rows up and down, a
selective blur (width-1)/2; the sharded bands exchange that halo before the operator."""
import numpy as np
import pytest

from conftest import make_pixels, to_device
from statistic_oracle import assert_same
from edge_blur_oracle import bilateral_pixels

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32


def single(im, image, step):
    if step[0] == "bilateralblur":
        return im.bilateral_blur_image(image, *step[1:])
    if step[0] == "selectiveblur":
        return im.selective_blur_image(image, *step[1:])
    return im.blur_image(image, *step[1:])


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_batch_edge_blurs(im, memory, dtype):
    pixels = [bilateral_pixels(90, 70, 4, dtype, seed=500 + i) for i in range(4)]
    chain = [("bilateralblur", 5, 7, 20.0, 3.0), ("selectiveblur", 0.0, 1.5, 6553.5)]
    images = [im.Image(p.copy() if memory == "host" else to_device(p)) for p in pixels]
    results = [image.like() for image in images]
    report = im.batch_images(chain, images, results, devices=2, streams_per_device=2)
    assert sum(report["images_per_device"]) == len(pixels)
    for p, result in zip(pixels, results):
        one = im.Image(to_device(p))
        for step in chain:
            one = single(im, one, step)
        assert_same(result.numpy(), one.numpy(), "batch bilateral + selective (%s)" % memory)


@pytest.mark.parametrize("devices", [2, 4])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("step", [("bilateralblur", 3, 3, 20.0, 3.0), ("bilateralblur", 5, 15, 200.0, 10.0),
                                  ("selectiveblur", 0.0, 1.5, 6553.5), ("selectiveblur", 3.0, 1.0, 20000.0)])
def test_sharded_edge_blurs(im, devices, dtype, step):
    """A 203-row frame: every band edge has the operator's halo across it."""
    px = make_pixels(203, 120, 4, dtype, seed=61, kind="smooth") + (dtype(300) if dtype == Q16 else np.float32(300))
    want = single(im, im.Image(to_device(px)), step).numpy()
    result, report = im.sharded_image([step], im.Image(px.copy()), devices=devices)
    assert report["devices"] == devices
    assert_same(result.numpy(), want, "sharded %s, %d bands" % (step, devices))
    # behind another stencil: the halo rows are exchanged between the bands
    chain = [step, ("blur", 0.0, 1.0), step]
    one = im.Image(to_device(px))
    for link in chain:
        one = single(im, one, link)
    result, report = im.sharded_image(chain, im.Image(px.copy()), devices=devices)
    assert report["halo_exchanges"] == 4 * (devices - 1)      # in front of the second and the third stencil
    assert_same(result.numpy(), one.numpy(), "sharded %s after blur, %d bands" % (step, devices))
