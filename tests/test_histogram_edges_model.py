"""CPU side of tests/test_gpu_histogram_edges.py: the expected values of its level-scan and mask cases are what the
reference computes, before any GPU is involved.

* oracle.restate's ContrastStretchImage / EqualizeImage against the compiled reference at every argument pair of part A
  (the tie frame and the one-bin frame included) and every mask of part C at 37 x 41, with the reference run twice
  (it is deterministic on them).  Where the two disagree the restatement is what gets fixed.
* the host LUT builders MhContrastStretchLUT / MhEqualizeLUT against the restatement on synthetic tables, at the same
  pairs, for both Quantum kinds.
"""
import numpy as np
import pytest

import imagemagick_amd
from oracle import restate as R

import test_gpu_histogram_edges as edges

Q16, HDRI = np.uint16, np.float32


def restated(px, op, mask=None):
    """The restatement under the reference's -channel string: per-channel tables unless the mask is the default one
    (ContrastStretch) or carries SyncChannels (Equalize); channels outside the mask keep their samples."""
    if op[0] == "equalize":
        out = R.equalize_image(px, sync_channels=mask is None or mask.endswith(",sync"))
    else:
        out = R.contrast_stretch_image(px, op[1], op[2], all_channels=mask is None)
    for c in edges.mask_arguments(imagemagick_amd, mask, px.shape[2])[1]:
        out[:, :, c] = px[:, :, c]
    return out


def pinned(refmod, px, op, mask=None):
    first = edges.reference(refmod, px, op, mask)
    again = edges.reference(refmod, px, op, mask)
    assert np.array_equal(edges.bits(first), edges.bits(again)), "the reference differs between two runs: %s %s" % (op, mask)
    want = restated(px, op, mask)
    differ = edges.bits(first) != edges.bits(want)
    assert not differ.any(), "restatement != reference for %s mask %s: %d bytes" % (op, mask, int(differ.sum()))
    return first


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels,kind", [(1, "random"), (2, "random"), (3, "random"), (4, "random"), (4, "smooth")])
def test_restatement_at_the_level_scan_edges(refmod, dtype, channels, kind):
    px = edges.frame(edges.SMALL, channels, dtype, kind, seed=7 + channels)
    n = edges.SMALL[0] * edges.SMALL[1]
    results = [pinned(refmod, px, edges.stretch(b, w)) for b, w in edges.level_pairs(n)]
    if dtype == HDRI:
        assert not results[2].any() and not results[3].any()       # black = 65536 as a float Quantum: every sample maps to 0
    else:
        assert results[2].any()                                   # ... and 0 as a Q16 one: stretched from level 0
    assert not np.array_equal(results[0], px)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 4])
def test_restatement_on_the_tie_frame(refmod, dtype, channels):
    px = edges.tie_frame(channels, dtype)
    n = edges.SMALL[0] * edges.SMALL[1]
    same = pinned(refmod, px, edges.stretch(100.0, float(n)))
    assert np.array_equal(same, pinned(refmod, px, edges.stretch(100.001, float(n))))
    assert not np.array_equal(same, pinned(refmod, px, edges.stretch(99.999, float(n))))
    same = pinned(refmod, px, edges.stretch(0.0, n - 100.0))
    assert np.array_equal(same, pinned(refmod, px, edges.stretch(0.0, n - 100.001)))
    assert not np.array_equal(same, pinned(refmod, px, edges.stretch(0.0, n - 99.999)))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [3, 4])
def test_restatement_on_the_one_bin_frame(refmod, dtype, channels):
    n = edges.SMALL[0] * edges.SMALL[1]
    px = edges.one_bin_frame(channels, dtype, False)
    assert np.array_equal(pinned(refmod, px, edges.stretch(2.0, n - 2.0)), px)         # black == white: untouched
    px = edges.one_bin_frame(channels, dtype, True)
    got = pinned(refmod, px, edges.stretch(2.0, n - 2.0), "RGB")
    assert [np.array_equal(got[:, :, c], px[:, :, c]) for c in range(3)] == [True, False, True]


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [3, 4])
def test_restatement_under_the_masks(refmod, dtype, channels):
    px = edges.frame(edges.SMALL, channels, dtype, "smooth", seed=3)
    n = edges.SMALL[0] * edges.SMALL[1]
    for mask in edges.STRETCH_MASKS:
        pinned(refmod, px, edges.stretch(0.03 * n, n - 0.02 * n), mask)
    for mask in edges.EQUALIZE_MASKS:
        pinned(refmod, px, edges.EQUALIZE, mask)
    for per_channel in (False, True):
        planted = edges.planted_frame(channels, dtype, False)
        mask = {3: "RGB", 4: "RGBA"}[channels] if per_channel else None
        pinned(refmod, planted, edges.stretch(0.02 * n, n - 0.01 * n), mask)
        pinned(refmod, planted, edges.EQUALIZE, mask)


# ----------------------------------------------------------------------------------- the host LUT builders
def synthetic_tables():
    """Three tables over the same 1517 pixels: the tie frame's counts (100 in the first and 100 in the last bin), a
    sparse one whose end bins are empty, and one bin that holds all but three pixels."""
    n = edges.SMALL[0] * edges.SMALL[1]
    rng = np.random.default_rng(5)
    tie = np.zeros(65536, dtype=np.int64)
    tie[0] = tie[65535] = 100
    np.add.at(tie, rng.integers(1000, 60000, n - 200), 1)
    sparse = np.zeros(65536, dtype=np.int64)
    np.add.at(sparse, rng.integers(300, 400, n // 2), 1)
    np.add.at(sparse, rng.integers(40000, 40010, n - n // 2), 1)
    one = np.zeros(65536, dtype=np.int64)
    one[30000], one[100], one[60000] = n - 3, 1, 2
    return n, [tie, sparse, one]


@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_host_lut_builders_at_the_level_scan_edges(im, dtype):
    hdri = dtype == HDRI
    n, tables = synthetic_tables()
    px = np.stack([np.repeat(np.arange(65536), t) for t in tables], axis=1).astype(dtype).reshape(1, n, 3)
    hist = np.stack(tables, axis=1).astype(np.uint64)
    own = R.scale_quantum_to_map(px, hdri)

    def apply(lut, mask):
        out = px.copy()
        for c in range(3):
            if (mask >> c) & 1:
                out[:, :, c] = R.clamp_to_quantum(lut[own[:, :, c], c], hdri)
        return out

    pairs = edges.level_pairs(n) + [(2.0, n - 2.0), (100.0, float(n)), (99.999, float(n)), (100.001, float(n)),
                                    (0.0, n - 100.0), (0.0, n - 99.999), (0.0, n - 100.001)]
    masks = set()
    for b, w in pairs:
        lut, mask = im.contrast_stretch_lut(hist, n, 1, b, w, 1 if hdri else 0)
        want = R.contrast_stretch_image(px, b, w, all_channels=False)
        assert np.array_equal(edges.bits(apply(lut, mask)), edges.bits(want)), (b, w)
        masks.add(mask)
    assert {0b111, 0b011} <= masks                                # (2, n-2) leaves the one-bin column alone
    lut, mask = im.equalize_lut(hist, 1 if hdri else 0)
    assert mask == 0b111
    assert np.array_equal(edges.bits(apply(lut, mask)), edges.bits(R.equalize_image(px, sync_channels=False)))
    # black == white: every pixel in bin 0
    zero = np.zeros((65536, 1), dtype=np.uint64)
    zero[0, 0] = n
    assert im.equalize_lut(zero, 1 if hdri else 0)[1] == 0
