"""FAST BlurImage on the work items whose staged window hangs over the image's left or right edge
(convolve_fused_hybrid.hip: the first and the last 64-column strip, in every segment).  Whether a thread loads its
four-column group whole or column by column, clamped, is decided per work item; the clamped columns are copies of
the edge column.  The mode's contract: within one level of the compiled reference, edges included."""
import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity

pytestmark = pytest.mark.gpu

Q16 = np.uint16
# one strip with both edges (1..64), a right-edge strip with 1 to 64 live columns (65..128, 129..193), windows
# that hang over by fewer and by more than four columns
WIDTHS = [1, 3, 4, 5, 39, 40, 63, 64, 65, 100, 128, 129, 143, 193]
HEIGHTS = [1, 16, 17, 40]
# taps -> sigma: shift = (taps-1)/2 = 3, 4, 5, 6 (every residue mod 4: how far a clamped group reaches into the
# image) and the headline kernel's 39
SIGMAS = {7: 0.8, 9: 1.0, 11: 1.2, 13: 1.4, 79: 10.0}


def frame(layout, rows, cols, seed):
    return make_pixels(rows, cols, 3 if layout == "rgb" else 4, Q16, seed=seed)     # (rgba: random alpha too)


def reference_blur(refmod, layout, px, sigma):
    if layout == "plain4":
        # four plain channels = the reference's RGB blur of the first three and its gray blur of the fourth
        rows, cols = px.shape[:2]
        return np.concatenate([refmod.RefImage(px[:, :, :3].copy()).blur(0.0, sigma).numpy(),
                               refmod.RefImage(px[:, :, 3].copy()).blur(0.0, sigma).numpy().reshape(rows, cols, 1)], axis=2)
    return refmod.RefImage(px).blur(0.0, sigma).numpy().reshape(px.shape)


def fast_blur(im, layout, px, sigma):
    dev = im.Image(to_device(px), has_alpha=False) if layout == "plain4" else im.Image(to_device(px))
    im.set_precision(im.PRECISION_FAST)
    try:
        return im.blur_image(dev, 0.0, sigma).numpy()
    finally:
        im.set_precision(im.PRECISION_EXACT)


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
@pytest.mark.parametrize("taps", sorted(SIGMAS))
def test_blur_fast_edge_items(im, refmod, layout, taps):
    """Every width x height of the lists above, one layout and one kernel a case: within +-1 level."""
    sigma = SIGMAS[taps]
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps
    failures = []
    for cols in WIDTHS:
        for rows in HEIGHTS:
            px = frame(layout, rows, cols, seed=1000 * taps + 7 * cols + rows)
            got = fast_blur(im, layout, px, sigma)
            try:
                assert_parity(got, reference_blur(refmod, layout, px, sigma), False,
                              "fast %s blur %dx%d, %d taps" % (layout, cols, rows, taps))
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "%d of %d shapes: %s" % (len(failures), len(WIDTHS) * len(HEIGHTS), "; ".join(failures[:5]))


@pytest.mark.parametrize("layout", ["rgba", "plain4", "rgb"])
def test_blur_fast_edge_items_uneven_segments(im, refmod, options, layout):
    """64 columns x 200 rows cut into three segments of 5, 5 and 3 blocks: one strip, both edges, in every segment."""
    options.set("MAGICKHIP_FUSED_SEGMENTS", "3")
    px = frame(layout, 200, 64, seed=64200)
    for taps in (11, 79):
        got = fast_blur(im, layout, px, SIGMAS[taps])
        assert_parity(got, reference_blur(refmod, layout, px, SIGMAS[taps]), False,
                      "fast %s blur 64x200 in three segments, %d taps" % (layout, taps))


def real_blur(px, taps, blend):
    """The blur's real values (float64) of a frame whose rows are all alike — the column pass of such a frame changes
    nothing, its taps sum to one — under the reference's edge rule: [columns, channels]."""
    row = px[0].astype(np.float64)
    cols, shift = row.shape[0], (len(taps) - 1) // 2
    at = np.clip(np.arange(cols)[:, None] - shift + np.arange(len(taps))[None, :], 0, cols - 1)
    window = row[at]                                                   # [column, tap, channel]
    if not blend:
        return np.einsum("t,xtc->xc", taps, window)
    alpha = np.einsum("t,xt->x", taps, window[:, :, 3])
    colour = np.einsum("t,xtc->xc", taps, window[:, :, :3] * window[:, :, 3:]) / np.maximum(alpha, 1e-300)[:, None]
    return np.concatenate([colour, alpha[:, None]], axis=1)


def test_blur_fast_edge_is_replicated(im):
    """Beyond the image the reference sees the edge column again (virtual pixels: edge).  A frame whose first and
    last columns are nothing like their neighbours (0 and 65535 beside mid levels), and the same frame with those
    columns written out `shift` times on either side: the results on the frame's own columns are the same, level for
    level.  FAST sums in f32 on the matrix cores, in an order that depends on where a column falls in its 16-column
    tile, and the padded frame's columns fall elsewhere: two such results agree to the f16 operands' 22 bits, not to
    the last bit.  Each is within 0.05 level of the real value (the kernel's whole error, convolve_fused_hybrid.hip),
    so they round alike wherever the real value is further than that from a rounding tie.  The rows are all alike,
    so the real values are known (real_blur), and the mid levels are the first of a fixed list that keep every one
    of them 0.06 level from a tie."""
    taps_count = 11
    sigma, shift = SIGMAS[taps_count], (taps_count - 1) // 2
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps_count
    taps = np.asarray(im.kernel_to_numpy("Blur:0x%g" % sigma)[0], dtype=np.float64).reshape(-1)
    assert taps.shape[0] == taps_count
    rows, cols = 40, 100
    px = None
    for t in range(4000):
        candidate = np.empty((1, cols, 4), dtype=np.uint16)
        candidate[:, :, :3] = 20000 + 7 * t
        candidate[:, :, 3] = 40000 + 3 * t
        candidate[:, 0, :] = 0
        candidate[:, -1, :] = 65535
        real = np.concatenate([real_blur(candidate, taps, False), real_blur(candidate, taps, True)])
        if np.abs(real - np.floor(real) - 0.5).min() >= 0.06:
            px = np.ascontiguousarray(np.repeat(candidate, rows, axis=0))
            break
    assert px is not None, "no candidate frame keeps every real value 0.06 level from a rounding tie"
    padded = np.ascontiguousarray(np.concatenate([np.repeat(px[:, :1], shift, axis=1), px,
                                                  np.repeat(px[:, -1:], shift, axis=1)], axis=1))
    for layout in ("rgba", "plain4"):
        got = fast_blur(im, layout, px, sigma)
        want = fast_blur(im, layout, padded, sigma)[:, shift:shift + cols]
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print("replicated edge, %s: max |diff| = %d, %d of %d differ" % (layout, d.max(), int((d > 0).sum()), d.size))
        assert d.max() == 0, "%s: the clamped columns are not the edge column: max |diff| = %d at %s" % (
            layout, d.max(), np.argwhere(d > 0)[:3].tolist())
        # ... and they are what the edge rule says: within the mode's one level of the real values
        assert np.abs(got[0].astype(np.float64) - real_blur(px, taps, layout == "rgba")).max() <= 1.0
