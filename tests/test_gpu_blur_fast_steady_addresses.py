"""FAST BlurImage around the steady state of INTERIOR work items (convolve_fused_hybrid.hip).  In the steady state a
stager forms no address: it fetches through a workgroup-uniform row base in scalar registers plus a 32-bit offset it
formed once, clamps no row — the steady range ends where the image's last segment would first fetch row H — and every
wave stores its row of the finished block through a scalar row base, whole where the strip has its 64 columns, under a
loop-invariant lane mask where it has fewer.  The steady body is compiled per kind of item: interior, edge with a full
strip, ragged strip.  The walk-phase tests use widths 64 and 65, where every item is an edge item; the frames here have
interior strips.

A strip s is interior when 64*s - shift >= 0 and 64*s - shift + 32*NC + 48 <= W: for 79 taps (NC = 3, shift 39) strip
2 becomes interior exactly at W = 233.  Widths 232 and 233: strip 2 on either side of that; 256: interior strips
followed by a full edge strip; 257: followed by a ragged strip of one column.  Heights of 8 to 12 blocks: the steady
range exists, the bottom clamp cuts it at different iterations, with and without a ragged last block.  The mode's
contract: within one level of the compiled reference — nothing skipped, nothing masked."""
import pytest

from conftest import assert_parity
from test_gpu_blur_edge_items import frame, reference_blur, fast_blur

pytestmark = pytest.mark.gpu

WIDTHS = [232, 233, 256, 257]
HEIGHTS = [128, 129, 160, 161, 176, 177]
# taps -> sigma: NC = (taps+46)/32 = 1, 2, 3
SIGMAS = {7: 0.8, 41: 5.0, 79: 10.0}


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("taps", sorted(SIGMAS))
def test_blur_fast_steady_addresses(im, refmod, layout, taps):
    """Every width x height of the lists above, one layout and one kernel a case: within +-1 level."""
    sigma = SIGMAS[taps]
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps
    assert (taps + 15 + 31) // 32 == {7: 1, 41: 2, 79: 3}[taps]
    failures = []
    for cols in WIDTHS:
        for rows in HEIGHTS:
            px = frame(layout, rows, cols, seed=5000 * taps + 13 * cols + rows)
            got = fast_blur(im, layout, px, sigma)
            try:
                assert_parity(got, reference_blur(refmod, layout, px, sigma), False,
                              "fast %s blur %dx%d, %d taps" % (layout, cols, rows, taps))
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "%d of %d shapes: %s" % (len(failures), len(WIDTHS) * len(HEIGHTS), "; ".join(failures[:5]))


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("segments", [2, 3])
def test_blur_fast_steady_addresses_segments(im, refmod, options, layout, segments):
    """256 columns x 208 rows = 13 blocks in two (7 and 6 blocks) and three (5, 5 and 3) forced segments: the upper
    segments' fetches never reach the image's last row, the lowest one's do."""
    options.set("MAGICKHIP_FUSED_SEGMENTS", str(segments))
    px = frame(layout, 208, 256, seed=256208 + segments)
    for taps in sorted(SIGMAS):
        got = fast_blur(im, layout, px, SIGMAS[taps])
        assert_parity(got, reference_blur(refmod, layout, px, SIGMAS[taps]), False,
                      "fast %s blur 256x208 in %d segments, %d taps" % (layout, segments, taps))
