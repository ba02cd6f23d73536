"""FAST BlurImage on the edge work items IN THE STEADY STATE (convolve_fused_hybrid.hip: fetch_steady of an edge item).
There a stager of the first or the last 64-column strip fetches its four clamped columns through four byte offsets
formed once in front of the walk (StagerLane) and a workgroup-uniform row base, where the fill and drain iterations
clamp per lane.  The edge tests of tests/test_gpu_blur_edge_items.py stop at 40 rows, three blocks, and never reach a
steady iteration: these frames have eight and nine.  The widths are the ones at which another form of that fetch would
go wrong first (a group of four or a pair of columns that is wider than the image, every W mod 4, ragged last strips,
an interior strip between edge strips): profiles/hybrid_edge_fetch_alpha_settle.md measured one and dropped it.  The
mode's contract: within one level of the compiled reference, nothing skipped or masked."""
import numpy as np
import pytest

from conftest import assert_parity
from test_gpu_blur_edge_items import SIGMAS, frame, reference_blur, fast_blur, real_blur

pytestmark = pytest.mark.gpu

# 8 and 9 blocks of 16 rows: two steady iterations of 79 taps, and a last block of one row
HEIGHTS = [128, 129]
# every W mod 4 (where the last group of four columns meets the edge); 1..7: images narrower than two groups of four
# columns, every column group clamped on one side or on both; 64: one strip with both edges, full; 65..67, 131, 193: a ragged last strip
# of one to three columns; 100, 143: ragged strips whose window hangs over by more than a group; 193, 257: an interior
# strip between edge strips (79 taps: from 233 columns; the short kernels: from three strips)
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 64, 65, 66, 67, 100, 131, 143, 193, 257]


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("taps", sorted(SIGMAS))
def test_blur_fast_edge_fetch_steady(im, refmod, layout, taps):
    """Every width x height of the lists above, one layout and one kernel a case (shifts 3, 4, 5, 6 and 39: every
    residue mod 4 of where a clamped group begins): within +-1 level."""
    sigma = SIGMAS[taps]
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps
    failures = []
    for cols in WIDTHS:
        for rows in HEIGHTS:
            px = frame(layout, rows, cols, seed=2000 * taps + 11 * cols + rows)
            got = fast_blur(im, layout, px, sigma)
            try:
                assert_parity(got, reference_blur(refmod, layout, px, sigma), False,
                              "fast %s blur %dx%d, %d taps" % (layout, cols, rows, taps))
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "%d of %d shapes: %s" % (len(failures), len(WIDTHS) * len(HEIGHTS), "; ".join(failures[:5]))


# ---------------------------------------------------------------------------------------------------------------------
# The replicated edge at 144 rows.  test_blur_fast_edge_is_replicated's frame — every row alike, the first and the last
# column nothing like their neighbours — must keep every real value 0.06 level from a rounding tie for its two FAST
# results to round alike.  One mid level for all channels and the edge columns at exactly 0 and 65535 find such a frame
# for 11 taps, where ten columns feel the edges; for 79 taps 78 columns do, in seven different values each, and no mid
# level keeps all of them clear.  So the frame is searched channel by channel and side by side: a channel's mid level
# m, then its left edge level among 0..63 (the columns near the left edge see only m and that level) and its right edge
# level among 65472..65535 — still nothing like the mid levels beside them.
MARGIN = 0.06
EDGE_LEVELS = 64


def clear_of_ties(values):
    return np.abs(values - np.floor(values) - 0.5).min(axis=0) >= MARGIN


def edge_rows(taps, cols, count, first_mid, alpha=None):
    """`count` rows [left level, mid, ..., mid, right level] of one channel whose real values (plain: the weighted
    sums; with `alpha`, that channel's row: the alpha-weighted colour) all keep MARGIN from a tie."""
    shift = (len(taps) - 1) // 2
    # what source column c weighs in column x under the reference's edge rule: [x, c]
    at = np.clip(np.arange(cols)[:, None] - shift + np.arange(len(taps))[None, :], 0, cols - 1)
    weigh = np.zeros((cols, cols))
    np.add.at(weigh, (np.arange(cols)[:, None], at), taps[None, :])
    opacity = np.ones(cols) if alpha is None else alpha
    below = weigh @ opacity
    half = cols // 2
    found = []
    for mid in range(first_mid, first_mid + 4000):
        row = np.full(cols, float(mid))
        for edge, side, levels in ((0, slice(0, half), np.arange(EDGE_LEVELS, dtype=np.float64)),
                                   (cols - 1, slice(half, cols), 65535.0 - np.arange(EDGE_LEVELS))):
            # every level of the edge column at once: [column of the side, level]
            above = (weigh @ (opacity * row))[side, None] + \
                weigh[side, edge, None] * opacity[edge] * (levels[None, :] - row[edge])
            good = np.flatnonzero(clear_of_ties(above / below[side, None]))
            if len(good) == 0:
                break
            row[edge] = levels[good[0]]
        else:
            found.append(row)
            if len(found) == count:
                return found
    raise AssertionError("no frame keeps every real value %g level from a rounding tie" % MARGIN)


def replicated_edge_frame(layout, rows, cols, taps):
    assert cols // 2 > (len(taps) - 1) // 2          # a column feels one edge only: the sides are searched apart
    if layout == "plain4":
        channels = edge_rows(taps, cols, 4, 20000)
    else:
        alpha = edge_rows(taps, cols, 1, 40000)[0]
        channels = edge_rows(taps, cols, 3, 20000, alpha) + [alpha]
    row = np.stack(channels, axis=1).astype(np.uint16).reshape(1, cols, 4)
    # (and by the existing test's own restatement)
    real = np.concatenate([real_blur(row, taps, False)[:, 3:] if layout == "rgba" else real_blur(row, taps, False),
                           real_blur(row, taps, True)[:, :3] if layout == "rgba" else np.empty((cols, 0))], axis=1)
    assert clear_of_ties(real.reshape(-1, 1)).all()
    return np.ascontiguousarray(np.repeat(row, rows, axis=0))


@pytest.mark.parametrize("taps_count", [11, 79])
def test_blur_fast_edge_is_replicated_in_the_steady_state(im, taps_count):
    """Beyond the image the reference sees the edge column again.  144 rows, nine blocks: the steady iterations of the
    frame's two strips (an edge item with a full strip, a ragged one) fetch clamped columns; the same frame with its edge columns
    written out `shift` times on either side has an interior strip, or edge strips whose windows hang over by other
    amounts.  The results on the frame's own columns are the same, level for level, and within the mode's one level of
    the real values."""
    sigma, shift = SIGMAS[taps_count], (taps_count - 1) // 2
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps_count
    taps = np.asarray(im.kernel_to_numpy("Blur:0x%g" % sigma)[0], dtype=np.float64).reshape(-1)
    assert taps.shape[0] == taps_count
    rows, cols = 144, 100
    for layout in ("rgba", "plain4"):
        px = replicated_edge_frame(layout, rows, cols, taps)
        padded = np.ascontiguousarray(np.concatenate([np.repeat(px[:, :1], shift, axis=1), px,
                                                      np.repeat(px[:, -1:], shift, axis=1)], axis=1))
        got = fast_blur(im, layout, px, sigma)
        want = fast_blur(im, layout, padded, sigma)[:, shift:shift + cols]
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print("replicated edge, %d taps, %s: max |diff| = %d, %d of %d differ" % (
            taps_count, layout, d.max(), int((d > 0).sum()), d.size))
        assert d.max() == 0, "%s: the clamped columns are not the edge column: max |diff| = %d at %s" % (
            layout, d.max(), np.argwhere(d > 0)[:3].tolist())
        assert np.abs(got[0].astype(np.float64) - real_blur(px, taps, layout == "rgba")).max() <= 1.0
