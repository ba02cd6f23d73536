"""FAST BlurImage where the store of a finished row changes hands between the tested body and the steady state
(convolve_fused_hybrid.hip).  Every wave stores one row of the block the column pass has just finished.  The steady
bodies read the wave's pixel of out_tile at the head of interval B, with the first operand reads behind barrier X, and
store it from in front of the row chain through a scalar row base that moves on by a block an iteration; fill and drain
read and store behind the chain, under the tests of the block and the image's edges.  (A form that held a staging wave's
row over barrier Y and stored it in the next interval A — the steady range's first iteration in the tested body, one
store behind the loop — was measured and dropped: profiles/hybrid_row_store_waits.md.  These are its tests too.)  What
can go wrong is a row stored twice with different content, a row never stored, or a row stored from a stale register —
all of them at the seams between the tested body and the steady state.

Heights, for 79 taps (NC = 3: the steady range begins at group 7 and ends where the fetch would first reach row H):
112 rows: a range of one iteration; 128 and 129: two; 144: three; 176: five.  Widths: 64 and 65 (edge items only; 65: a ragged strip of one column),
169 (the narrowest frame whose strip 1 is interior: 64 - 39 + 144 <= W), 200 (an edge strip, an interior strip, a full
edge strip and a ragged strip of eight columns).  200 columns x 528 rows is 33 blocks in two segments of 17 and 16: the
second begins at row 272, its source rows from 233 on lie inside the image from the first group.

Every frame is blurred into a destination filled with 65535 beforehand.  The samples are at most 60000, a blurred
sample is a weighted mean of samples (of colours, under alpha weights), so no result within one level of the reference
is 65535: a pixel that keeps the filling was never stored.  The mode's contract: within one level of the compiled
reference on every sample."""
import numpy as np
import pytest

from conftest import to_device, assert_parity
from test_gpu_blur_edge_items import reference_blur

pytestmark = pytest.mark.gpu

WIDTHS = [64, 65, 169, 200]
HEIGHTS = [112, 128, 129, 144, 176]
SHAPES = [(rows, cols) for cols in WIDTHS for rows in HEIGHTS] + [(528, 200)]
# taps -> sigma: NC = (taps+46)/32 = 3 (BlurImage 0x10, the headline kernel) and 1
SIGMAS = {7: 0.8, 79: 10.0}
CEILING, FILLING = 60000, 65535


def frame(layout, rows, cols, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.integers(0, CEILING + 1, (rows, cols, 3 if layout == "rgb" else 4), dtype=np.uint16))


def fast_blur_into_filled(im, layout, px, sigma):
    import torch
    src = im.Image(to_device(px), has_alpha=False) if layout == "plain4" else im.Image(to_device(px))
    out = src.like()
    out.pixels.view(torch.int16).fill_(-1)                             # 65535 in every sample
    assert int(out.numpy().min()) == FILLING
    im.set_precision(im.PRECISION_FAST)
    try:
        return im.blur_image(src, 0.0, sigma, out=out).numpy()
    finally:
        im.set_precision(im.PRECISION_EXACT)


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("taps", sorted(SIGMAS))
def test_blur_fast_row_store(im, refmod, layout, taps):
    """Every shape of the list above, one layout and one kernel a case: every sample stored, within +-1 level."""
    sigma = SIGMAS[taps]
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps
    assert (taps + 15 + 31) // 32 == {7: 1, 79: 3}[taps]
    failures = []
    for rows, cols in SHAPES:
        px = frame(layout, rows, cols, seed=7000 * taps + 17 * cols + rows)
        got = fast_blur_into_filled(im, layout, px, sigma)
        what = "fast %s blur %dx%d, %d taps" % (layout, cols, rows, taps)
        try:
            kept = got == FILLING
            assert not kept.any(), "%s: %d samples keep the destination's filling, rows %s" % (
                what, int(kept.sum()), sorted(set(np.argwhere(kept)[:, 0].tolist()))[:8])
            assert_parity(got, reference_blur(refmod, layout, px, sigma), False, what)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "%d of %d shapes: %s" % (len(failures), len(SHAPES), "; ".join(failures[:5]))
