"""The NumPy restatement of KuwaharaImage's selection (tests/kuwahara_oracle.py) against the compiled
reference, bit for bit, and the conditions the GPU tests' inputs must meet: on the noise frames every
quadrant is chosen often, on flat frames the tie rule decides.  No GPU needed."""
import numpy as np
import pytest

from statistic_oracle import assert_same
from kuwahara_oracle import (SHAPES, cases, CHANNELS, ref_kuwahara, restate, noise, constant, flat_blocks,
                             plain4_reference)

Q16, HDRI = np.uint16, np.float32


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("shape", [(61, 97), (23, 40)])
def test_restatement_equals_the_reference(refmod, shape, dtype, channels):
    px = noise(shape[0], shape[1], channels, dtype)
    for radius in (0, 1, 2, 3, 4):
        blurred = refmod.RefImage(px).blur(radius, 1.5).numpy()
        got, _ = restate(blurred, radius)
        want = ref_kuwahara(refmod, refmod.RefImage(px), radius, 1.5).numpy()
        assert_same(got, want, "restatement %s c%d radius %g %s" % (shape, channels, radius, dtype.__name__))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_every_quadrant_is_chosen_on_the_noise_frames(refmod, dtype):
    """A condition on the inputs of tests/test_gpu_kuwahara.py: by symmetry every quadrant is chosen
    on a quarter of the pixels of an i.i.d. frame; at least 10 % each is asked wherever the frame is
    larger than the windows and the windows hold more than one pixel.  A kernel that always picks one
    quadrant cannot pass the parity tests on such frames."""
    checked = 0
    for index, shape in enumerate(SHAPES):
        for radius, sigma, layout in cases(index):
            w = int(radius) + 1
            if w < 2 or min(shape) < 2 * w or layout == "plain4":
                continue
            px = noise(shape[0], shape[1], CHANNELS[layout], dtype)
            blurred = refmod.RefImage(px).blur(radius, sigma).numpy()
            _, quadrant = restate(blurred, radius)
            share = np.bincount(quadrant.ravel(), minlength=4) / quadrant.size
            assert share.min() >= 0.10, (shape, radius, sigma, layout, share)
            checked += 1
    assert checked >= 10


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_ties_keep_the_earliest_quadrant(refmod, dtype):
    for radius in (1, 2, 4):
        px = constant(40, 50, 3, dtype)
        blurred = refmod.RefImage(px).blur(radius, 1.5).numpy()
        got, quadrant = restate(blurred, radius)
        assert (quadrant == 0).all(), "a constant frame: all four variances are 0"
        assert_same(got, ref_kuwahara(refmod, refmod.RefImage(px), radius, 1.5).numpy(), "constant frame")
        # flat 32 x 32 blocks, unblurred: inside a block all four variances are 0 as well
        px = flat_blocks(96, 128, 3, dtype)
        w = radius + 1
        got, quadrant = restate(px, radius)
        inside = np.zeros(px.shape[:2], dtype=bool)
        for y in range(0, 96, 32):
            for x in range(0, 128, 32):
                inside[y + w - 1:y + 32 - (w - 1), x + w - 1:x + 32 - (w - 1)] = True
        assert inside.any() and (quadrant[inside] == 0).all()
        assert (quadrant != 0).any(), "next to a block edge another quadrant is the calm one"
        # ... and through the whole operator, blur included
        blurred = refmod.RefImage(px).blur(radius, 0.5).numpy()
        got, _ = restate(blurred, radius)
        assert_same(got, ref_kuwahara(refmod, refmod.RefImage(px), radius, 0.5).numpy(), "flat blocks")


def test_plain_four_channel_restatement(refmod):
    px = noise(23, 40, 4, Q16)
    want = plain4_reference(refmod, px, 2, 1.5)
    assert want.shape == px.shape
