"""MH_OP_KUWAHARA in MagickHipBatchImages and MagickHipShardedImage: the same bits as one call of the
operator and as the compiled reference.  The operator reaches the blur's half width plus its own
window side in rows; the sharded bands exchange that halo before it."""
import numpy as np
import pytest

from conftest import to_device
from statistic_oracle import assert_same
from kuwahara_oracle import noise, ref_kuwahara

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_batch_kuwahara(im, refmod, memory, dtype):
    pixels = [noise(48, 64, 4, dtype, seed=700 + i) for i in range(6)]
    chain = [("kuwahara", 2, 1.5)]
    images = [im.Image(p.copy() if memory == "host" else to_device(p)) for p in pixels]
    results = [image.like() for image in images]
    report = im.batch_images(chain, images, results, devices=2, streams_per_device=2)
    assert report["devices"] == 2 and sum(report["images_per_device"]) == len(pixels)
    for p, result in zip(pixels, results):
        one = im.kuwahara_image(im.Image(to_device(p)), 2, 1.5).numpy()
        assert_same(result.numpy(), one, "batch kuwahara (%s)" % memory)
        assert_same(one, ref_kuwahara(refmod, refmod.RefImage(p), 2, 1.5).numpy(), "single kuwahara")


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_sharded_kuwahara(im, refmod, dtype):
    """80 rows in 3 bands, radius 3: windows and blur taps cross every band edge."""
    px = noise(80, 96, 4, dtype, seed=61)
    want = ref_kuwahara(refmod, refmod.RefImage(px), 3, 1.5).numpy()
    assert_same(im.kuwahara_image(im.Image(to_device(px)), 3, 1.5).numpy(), want, "single kuwahara")
    result, report = im.sharded_image([("kuwahara", 3, 1.5)], im.Image(px.copy()), devices=3)
    assert report["devices"] == 3
    assert_same(result.numpy(), want, "sharded kuwahara, 3 bands")
    # behind another stencil: the halo rows are exchanged between the bands
    chain = [("blur", 0.0, 1.0), ("kuwahara", 3, 1.5)]
    one = im.kuwahara_image(im.blur_image(im.Image(to_device(px)), 0.0, 1.0), 3, 1.5).numpy()
    result, report = im.sharded_image(chain, im.Image(px.copy()), devices=3)
    assert report["halo_exchanges"] >= 2
    assert_same(result.numpy(), one, "sharded blur + kuwahara, 3 bands")
