"""FAST BlurImage at the boundaries of the walk's phases (convolve_fused_hybrid.hip).  The walk over a work item's
16-row groups is compiled per set of wave roles and, in each, twice: a steady-state body that tests nothing about
the group index, and the tested body of fill and drain.  The steady range is NG+1 <= g <= ngroups-2 — nblocks-3
iterations, none below four blocks of 16 rows — and begins after 3, 5 and 7 groups for kernels of one, two and three
32-sample chunks (NC).  The frames here are the smallest that put an item on either side of each boundary: 3 to 6
blocks, a full and a ragged 64-column strip, every layout (alpha-weighted: alpha waves; four plain channels: no alpha
role; RGB: waves 12..15 neither row nor alpha waves), every NC, and forced segments, whose own fill recomputes the
halo groups.  The mode's contract: within one level of the compiled reference — nothing skipped, nothing masked."""
import numpy as np
import pytest

from conftest import assert_parity
from test_gpu_blur_edge_items import frame, reference_blur, fast_blur

pytestmark = pytest.mark.gpu

# nblocks = ceil(rows/16) = 3, 4, 4, 5, 5, 6: zero, one, one, two, two, three steady iterations
HEIGHTS = [48, 49, 64, 65, 80, 81]
# one full strip; a full strip and a ragged one of a single column
WIDTHS = [64, 65]
# taps -> sigma: NC = (taps+46)/32 = 1, 2, 3
SIGMAS = {7: 0.8, 41: 5.0, 79: 10.0}


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("taps", sorted(SIGMAS))
def test_blur_fast_walk_phases(im, refmod, layout, taps):
    """Every height x width of the lists above, one layout and one kernel a case: within +-1 level."""
    sigma = SIGMAS[taps]
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps
    assert (taps + 15 + 31) // 32 == {7: 1, 41: 2, 79: 3}[taps]
    failures = []
    for rows in HEIGHTS:
        for cols in WIDTHS:
            px = frame(layout, rows, cols, seed=3000 * taps + 11 * cols + rows)
            got = fast_blur(im, layout, px, sigma)
            try:
                assert_parity(got, reference_blur(refmod, layout, px, sigma), False,
                              "fast %s blur %dx%d, %d taps" % (layout, cols, rows, taps))
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "%d of %d shapes: %s" % (len(failures), len(HEIGHTS) * len(WIDTHS), "; ".join(failures[:5]))


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("segments", [3, 4])
def test_blur_fast_walk_phases_segments(im, refmod, options, layout, segments):
    """64 columns x 208 rows = 13 blocks, cut into three segments (5, 5 and 3 blocks) and into four (4, 4, 4 and 1):
    items on both sides of the four blocks at which the steady state begins, each with a fill of its own."""
    options.set("MAGICKHIP_FUSED_SEGMENTS", str(segments))
    px = frame(layout, 208, 64, seed=64208 + segments)
    for taps in sorted(SIGMAS):
        got = fast_blur(im, layout, px, SIGMAS[taps])
        assert_parity(got, reference_blur(refmod, layout, px, SIGMAS[taps]), False,
                      "fast %s blur 64x208 in %d segments, %d taps" % (layout, segments, taps))
