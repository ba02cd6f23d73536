"""MH_OP_STATISTIC in MagickHipBatchImages and MagickHipShardedImage: the same bits as one
MagickHipStatisticImage call.  A statistic reaches H/2 rows up and H-1-H/2 down; the sharded
bands exchange that halo before the operator."""
import numpy as np
import pytest

from conftest import make_pixels, to_device
from statistic_oracle import assert_same

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_batch_statistic(im, memory, dtype):
    pixels = [make_pixels(90, 70, 4, dtype, seed=500 + i) for i in range(4)]
    chain = [("statistic", "Median", 5, 5), ("statistic", "StandardDeviation", 3, 4)]
    images = [im.Image(p.copy() if memory == "host" else to_device(p)) for p in pixels]
    results = [image.like() for image in images]
    report = im.batch_images(chain, images, results, devices=2, streams_per_device=2)
    assert sum(report["images_per_device"]) == len(pixels)
    for p, result in zip(pixels, results):
        one = im.statistic_image(im.Image(to_device(p)), "Median", 5, 5)
        want = im.statistic_image(one, "StandardDeviation", 3, 4).numpy()
        assert_same(result.numpy(), want, "batch median + stddev (%s)" % memory)


@pytest.mark.parametrize("devices", [2, 4])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("statistic,width,height", [("Median", 3, 3), ("Mode", 4, 7), ("Mean", 9, 9),
                                                    ("Maximum", 2, 6), ("NonPeak", 5, 11)])
def test_sharded_statistic(im, devices, dtype, statistic, width, height):
    px = make_pixels(203, 120, 4, dtype, seed=61)
    want = im.statistic_image(im.Image(to_device(px)), statistic, width, height).numpy()
    chain = [("statistic", statistic, width, height), ("blur", 0.0, 1.0), ("statistic", statistic, width, height)]
    result, report = im.sharded_image(chain[:1], im.Image(px.copy()), devices=devices)
    assert report["devices"] == devices
    assert_same(result.numpy(), want, "sharded %s %dx%d, %d bands" % (statistic, width, height, devices))
    # a statistic behind another stencil: its halo rows are exchanged between the bands
    one = im.Image(to_device(px))
    for step in chain:
        one = im.statistic_image(one, *step[1:]) if step[0] == "statistic" else im.blur_image(one, *step[1:])
    result, report = im.sharded_image(chain, im.Image(px.copy()), devices=devices)
    assert report["halo_exchanges"] == 4 * (devices - 1)      # in front of the second and the third stencil
    assert_same(result.numpy(), one.numpy(), "sharded %s after blur, %d bands" % (statistic, devices))
