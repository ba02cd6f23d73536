"""The NumPy restatement of CLAHEImage's core (tests/clahe_oracle.py) against the compiled reference,
bit for bit, on frames declared Lab (no conversion runs) for every case of tests/test_gpu_clahe.py;
that the reference survives each of those shapes; and the conditions the case list must meet.  No
GPU needed."""
import numpy as np
import pytest

from statistic_oracle import assert_same
from clahe_oracle import (SHAPES, BINS, CLIPS, INPUTS, cases, reference, restate_frame, noise, float_specials,
                          table_fits, clip_histogram, geometry)

Q16, HDRI = np.uint16, np.float32


def test_the_case_list_covers_every_axis_and_fits_the_table_rule():
    seen = [set(), set(), set()]
    for index, (rows, cols, width, height) in enumerate(SHAPES):
        for case in cases(index):
            for axis, value in enumerate(case):
                seen[axis].add(value)
            assert table_fits(rows, cols, case[2], Q16, width, height, case[0]), (index, case)
    assert seen[0] == set(BINS) and seen[1] == set(CLIPS) and seen[2] == {3, 4}


def test_the_shapes_are_what_their_comments_say():
    assert geometry(16, 16, 0, 0) == (2, 2, 0, 0)
    assert geometry(61, 97, 16, 16) == (16, 16, 15, 3)           # 7 columns left, 8 right
    assert geometry(33, 50, 7, 5) == (7, 5, 6, 2)
    assert geometry(20, 30, 64, 64) == (64, 64, 34, 44)
    assert geometry(1030, 2051, 0, 0) == (256, 128, 253, 122)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("index", range(len(SHAPES)))
def test_restatement_equals_the_reference(refmod, index, dtype):
    rows, cols, width, height = SHAPES[index]
    for number_bins, clip_limit, channels in cases(index):
        px = noise(rows, cols, channels, dtype)
        want = reference(refmod, px, "Lab", width, height, number_bins, clip_limit)
        got = restate_frame(px, width, height, number_bins, clip_limit)
        assert_same(got, want, "restatement %s bins %d clip %g %s" % (SHAPES[index], number_bins, clip_limit, dtype.__name__))
        if clip_limit != 1.0:
            assert (want[..., 0] != px[..., 0]).any()


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_restatement_on_the_structured_inputs(refmod, name, dtype):
    for (rows, cols, width, height), number_bins, clip_limit in [((61, 97, 16, 16), 128, 2.0), ((33, 50, 7, 5), 3, 1.5),
                                                                 ((64, 64, 8, 8), 255, 0.5)]:
        px = INPUTS[name](rows, cols, 4, dtype)
        want = reference(refmod, px, "Lab", width, height, number_bins, clip_limit)
        assert_same(restate_frame(px, width, height, number_bins, clip_limit), want, "%s %dx%d" % (name, rows, cols))


def test_restatement_on_float_specials(refmod):
    for (rows, cols, width, height), number_bins, clip_limit in [((61, 97, 16, 16), 128, 2.0), ((33, 50, 7, 5), 3, 1.0)]:
        px = float_specials(rows, cols, 3)
        assert (px[..., 0] < 0).any() and (px[..., 0] > 65535).any()
        want = reference(refmod, px, "Lab", width, height, number_bins, clip_limit)
        assert_same(restate_frame(px, width, height, number_bins, clip_limit), want, "float specials")
        assert (want[..., 0] != px[..., 0]).any()


def test_the_redistribution_sweeps_are_exercised():
    """Conditions on the inputs: a constant tile leaves more excess than bins behind the second loop
    (whole stride-1 sweeps), and a remainder below the bin count (strided sweeps)."""
    histogram = [0] * 128
    histogram[60] = 256 * 128
    limit = int(2.0 * 256 * 128 / 128)
    out = clip_histogram(limit, list(histogram))
    assert out[60] == limit and min(out) > 0 and sum(out) == 256 * 128
    assert len(set(out)) > 2, "the strided remainder reached only some bins"
