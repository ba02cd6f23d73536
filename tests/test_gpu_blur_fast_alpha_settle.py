"""FAST BlurImage where the alpha waves' rare path runs inside the steady state (convolve_fused_hybrid.hip: the ALPHA
branch of an iteration).  The row pass's alpha sums are exact integers with a certificate; a sum the certificate cannot
decide — within 3e-7 level of a rounding tie for 79 taps — is settled by the whole wave (settle_doubtful_pixels), in a
branch between the certificate and the publication of the levels and weights that fifteen other waves wait for; only a
frame that has such pixels shows whether what is published is the settled level.  Random frames have none
(6e-7 of the pixels), and the alternating alpha of the tie tests lies 8e-6 from a tie: here the alpha sums are PUT on
ties.  One alpha row of small levels, the same in every row; at a few target columns three samples of the window are
moved by a few levels, found by a meet-in-the-middle search over the window's columns, so that the row pass's alpha sum
lies within 3e-9 of n + 0.5.  Small alpha levels and random colours: an intermediate alpha level that is one off moves
the colours by hundreds of levels.  The contract: within one level of the compiled reference."""
import functools

import numpy as np
import pytest

from conftest import assert_parity
from test_gpu_blur_edge_items import reference_blur, fast_blur

pytestmark = pytest.mark.gpu

SIGMAS = {41: 5.0, 79: 10.0}
# columns x rows -> the target columns: one in strip 0, one in an interior strip (64..127: its window stays inside the
# image for both kernels), one in the last strip, which is ragged (257: the one column 256; 233: 41 columns); more than
# 79 columns apart, so that no sample belongs to two targets' windows
SHAPES = {(257, 160): (20, 120, 256), (233, 129): (20, 110, 215)}
# How near a tie the search puts a sum.  Within 1e-8 is what makes a pixel one the fp64 recomputation cannot decide
# either; but "every target is settled" needs the certificate to doubt it, and the certificate's window is the taps'
# quantisation error e plus 4e-9 (plan_exact_taps: 3.1e-7 for 79 taps, under 1e-8 for 41).  The device's sum lies
# within e of the real one, so a real sum within 3e-9 of the tie is doubted whatever the taps.
TIE_WINDOW = 3.0e-9
BASE_LEVELS = 8                                    # the alpha row: levels 0..7
TOP_LEVEL = 15                                     # a moved sample stays a small level


def effective_weights(taps, x, cols):
    """What each source column weighs in the row pass's sum of column x under the reference's edge rule."""
    shift = (len(taps) - 1) // 2
    at = np.clip(x - shift + np.arange(len(taps)), 0, cols - 1)
    return np.bincount(at, weights=taps, minlength=cols)


def alpha_sums(row, taps):
    return np.array([effective_weights(taps, x, row.shape[0]) @ row for x in range(row.shape[0])])


def put_on_tie(row, taps, x, rng):
    """Moves three samples of column x's window so that its alpha sum lies within TIE_WINDOW of some n + 0.5.  The
    sums three moves can reach lie some 1e-8 apart: where none of them fits, the window's levels are drawn again."""
    weight = effective_weights(taps, x, row.shape[0])
    sources = np.flatnonzero(weight)
    for attempt in range(400):
        moved = three_moves(row, weight, sources)
        if moved is not None:
            return moved
        row = row.copy()
        row[sources] = rng.integers(0, BASE_LEVELS, len(sources))
    raise AssertionError("no three moves put column %d's alpha sum on a tie" % x)


def three_moves(row, weight, sources):
    # a move: (column, by how many levels) -> what it adds to the sum
    moves = [(c, d) for c in sources for d in range(-int(row[c]), TOP_LEVEL - int(row[c]) + 1) if d != 0]
    column = np.array([c for c, _ in moves])
    added = np.array([weight[c] * d for c, d in moves])
    first, second = np.triu_indices(len(moves), 1)
    apart = column[first] != column[second]
    first, second = first[apart], second[apart]
    pairs = added[first] + added[second]
    order = np.argsort(pairs)
    pairs, first, second = pairs[order], first[order], second[order]
    base = float(weight @ row)
    for n in range(0, TOP_LEVEL):
        wanted = (n + 0.5 - base) - added          # what a pair has to add beside each single move
        at = np.clip(np.searchsorted(pairs, wanted), 1, len(pairs) - 1)
        for k in (at - 1, at):
            close = np.flatnonzero(np.abs(pairs[k] - wanted) < TIE_WINDOW)
            for third in close:
                trio = (third, first[k[third]], second[k[third]])
                if len({int(column[i]) for i in trio}) < 3:
                    continue
                moved = row.copy()
                for i in trio:
                    moved[column[i]] += moves[i][1]
                if abs(float(weight @ moved) - (n + 0.5)) < TIE_WINDOW:
                    return moved
    return None


@functools.lru_cache(maxsize=None)
def alpha_row(cols, taps_key, targets, seed):
    """The alpha row (float64 levels) and how far its sums lie from a rounding tie; targets = (): a row whose sums all
    keep 1e-5 from one (a hundred times the certificate's window)."""
    taps = np.asarray(taps_key)
    for attempt in range(64):
        rng = np.random.default_rng(seed + attempt)
        row = rng.integers(0, BASE_LEVELS, cols).astype(np.float64)
        for x in targets:
            row = put_on_tie(row, taps, x, rng)
        sums = alpha_sums(row, taps)
        distance = np.abs(sums - np.floor(sums) - 0.5)
        if targets:
            assert (distance[list(targets)] < TIE_WINDOW).all()
            return row, distance
        if distance.min() > 1.0e-5:
            return row, distance
    raise AssertionError("no alpha row keeps every sum away from the ties")


def settle_frame(cols, rows, taps, targets, seed):
    row, distance = alpha_row(cols, tuple(taps.tolist()), tuple(targets), seed)
    px = np.random.default_rng(seed + 1000).integers(0, 65536, (rows, cols, 4), dtype=np.uint16)
    px[:, :, 3] = row.astype(np.uint16)[None, :]
    return np.ascontiguousarray(px), distance


def counted_blur(im, px, sigma):
    lib = im.load()
    lib.MhExactBlurRecomputed(1)
    try:
        got = fast_blur(im, "rgba", px, sigma)
    finally:
        recomputed = lib.MhExactBlurRecomputed(0)
    return got, int(recomputed)


@pytest.mark.parametrize("taps_count", sorted(SIGMAS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_blur_fast_alpha_on_ties_in_the_steady_state(im, refmod, shape, taps_count):
    """Three columns of every row on a tie of the intermediate alpha: each of them is settled (the count says so), in
    the tested body and in all three steady bodies, and the result is within one level of the reference."""
    (cols, rows), sigma = shape, SIGMAS[taps_count]
    assert im.optimal_kernel_width_1d(0.0, sigma) == taps_count
    taps = np.asarray(im.kernel_to_numpy("Blur:0x%g" % sigma)[0], dtype=np.float64).reshape(-1)
    targets = SHAPES[shape]
    px, distance = settle_frame(cols, rows, taps, targets, seed=100 * taps_count + cols)
    print("alpha sums of the targets: %s from a tie" % ", ".join("%.1e" % distance[x] for x in targets))
    got, recomputed = counted_blur(im, px, sigma)
    print("%dx%d, %d taps: %d pixels settled (%d rows x %d targets)" % (cols, rows, taps_count, recomputed, rows, len(targets)))
    assert_parity(got, reference_blur(refmod, "rgba", px, sigma), False,
                  "fast rgba blur %dx%d, %d taps, alpha sums on ties" % (cols, rows, taps_count))
    assert recomputed >= rows * len(targets), recomputed


@pytest.mark.parametrize("taps_count", sorted(SIGMAS))
def test_blur_fast_alpha_away_from_ties_settles_nothing(im, refmod, taps_count):
    """The same kind of frame with no column moved and every alpha sum 1e-5 from a tie: nothing, or next to nothing,
    takes the rare path."""
    (cols, rows), sigma = (257, 160), SIGMAS[taps_count]
    taps = np.asarray(im.kernel_to_numpy("Blur:0x%g" % sigma)[0], dtype=np.float64).reshape(-1)
    assert taps.shape[0] == taps_count
    px, distance = settle_frame(cols, rows, taps, (), seed=100 * taps_count + cols)
    got, recomputed = counted_blur(im, px, sigma)
    print("%dx%d, %d taps: nearest alpha sum %.1e from a tie, %d pixels settled" % (cols, rows, taps_count, distance.min(), recomputed))
    assert_parity(got, reference_blur(refmod, "rgba", px, sigma), False,
                  "fast rgba blur %dx%d, %d taps, alpha sums away from ties" % (cols, rows, taps_count))
    assert recomputed * 16 < rows, recomputed
