"""The NumPy restatement of SampleImage and ScaleImage (scale_oracle.py) against the compiled reference,
bit for bit on both Quantum builds, and the library's host plans against the Python plans.  No GPU."""
import numpy as np
import pytest

from statistic_oracle import assert_same
from scale_oracle import (BIG, CHANNELS, EXTREME, GEOMETRIES, LAYOUTS, MASKS, SAMPLE_OFFSETS, frame, layout_has_alpha,
                          negative_alpha_float, offset_percent, out_of_range_float, plan_columns, plan_rows, ref_image,
                          ref_sample, ref_scale, restate_sample, restate_scale, sample_offsets)

Q16, HDRI = np.uint16, np.float32


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_restatement_equals_the_reference(refmod, layout, dtype):
    for index, ((rows, cols), (to_rows, to_cols)) in enumerate(GEOMETRIES):
        # a third of the alpha frames carry fully transparent pixels
        px = frame(layout, rows, cols, dtype, seed=index, transparent=0.3 if index % 3 == 0 else 0.0)
        what = "%dx%d -> %dx%d %s %s" % (rows, cols, to_rows, to_cols, layout, px.dtype.name)
        assert_same(restate_scale(px, to_rows, to_cols, layout_has_alpha(layout)),
                    ref_scale(refmod, ref_image(refmod, px), to_rows, to_cols).numpy(), "scale " + what)
        assert_same(restate_sample(px, to_rows, to_cols),
                    ref_sample(refmod, ref_image(refmod, px), to_rows, to_cols).numpy(), "sample " + what)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("mask", list(MASKS))
def test_channel_masks(refmod, mask, dtype):
    """A channel the mask leaves out carries Copy without Blend: scaled unweighted, stored undivided."""
    blend = tuple(c for c in range(3) if c not in MASKS[mask][1])
    for (rows, cols), (to_rows, to_cols) in GEOMETRIES[:7] + [GEOMETRIES[10]]:
        px = frame("rgba", rows, cols, dtype, seed=31, transparent=0.3)
        what = "mask %s %dx%d -> %dx%d %s" % (mask, rows, cols, to_rows, to_cols, px.dtype.name)
        assert_same(restate_scale(px, to_rows, to_cols, True, blend),
                    ref_scale(refmod, ref_image(refmod, px, mask=mask), to_rows, to_cols).numpy(), "scale " + what)
        assert_same(restate_sample(px, to_rows, to_cols),
                    ref_sample(refmod, ref_image(refmod, px, mask=mask), to_rows, to_cols).numpy(), "sample " + what)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_float_frames_out_of_range_and_negative_alpha(refmod, layout):
    for (rows, cols), (to_rows, to_cols) in GEOMETRIES[:7] + [GEOMETRIES[10]]:
        frames = [out_of_range_float(rows, cols, CHANNELS[layout])]
        if layout_has_alpha(layout):
            frames.append(negative_alpha_float(rows, cols, CHANNELS[layout]))
        for px in frames:
            what = "%dx%d -> %dx%d %s" % (rows, cols, to_rows, to_cols, layout)
            assert_same(restate_scale(px, to_rows, to_cols, layout_has_alpha(layout)),
                        ref_scale(refmod, ref_image(refmod, px), to_rows, to_cols).numpy(), "scale " + what)


def _flatten(plan):
    counts = np.array([len(terms) for terms in plan], dtype=np.uint32)
    indices = np.array([source for terms in plan for source, _ in terms], dtype=np.int32)
    weights = np.array([weight for terms in plan for _, weight in terms], dtype=np.float64)
    return counts, indices, weights


def _same_plan(im, source, destination, axis):
    got = im.scale_image_plan(source, destination, axis)
    assert got is not None, (source, destination, axis)
    want = (plan_rows, plan_columns)[axis](source, destination)
    if want is None:
        assert got[0].sum() == 0 and got[1].size == 0, (source, destination, axis)
        return
    counts, indices, weights = _flatten(want)
    what = "%d -> %d axis %d" % (source, destination, axis)
    assert np.array_equal(got[0], counts), what
    assert np.array_equal(got[1], indices), what
    assert np.array_equal(got[2].view(np.uint64), weights.view(np.uint64)), what      # exact doubles


def test_host_plan_equals_the_python_plan():
    """MhScaleImagePlan term for term: sources, weights as exact doubles, order."""
    import imagemagick_amd as im
    im.load()
    for source in range(1, 129):
        for destination in range(1, 129):
            for axis in (0, 1):
                _same_plan(im, source, destination, axis)
    for (rows, cols), (to_rows, to_cols) in (BIG, EXTREME, ((8192, 2000), (819, 3)), ((2048, 3), (8192, 2000))):
        _same_plan(im, rows, to_rows, 0)
        _same_plan(im, cols, to_cols, 1)


@pytest.mark.parametrize("offset", SAMPLE_OFFSETS)
def test_sample_offsets_equal_the_reference(refmod, offset):
    """A frame whose samples are their own position: the reference's result spells its offsets out."""
    import imagemagick_amd as im
    im.load()
    for (rows, cols), (to_rows, to_cols) in [g for g in GEOMETRIES if g[0][0] * g[0][1] <= 65536]:
        px = np.arange(rows * cols, dtype=np.uint16).reshape(rows, cols, 1)
        got = ref_sample(refmod, ref_image(refmod, px), to_rows, to_cols, offset).numpy()[..., 0].astype(np.int64)
        ox, oy = offset_percent(offset)
        what = "%dx%d -> %dx%d offset %s" % (rows, cols, to_rows, to_cols, offset)
        for python, library in ((sample_offsets(cols, to_cols, ox), im.sample_image_offsets(cols, to_cols, ox)),
                                (sample_offsets(rows, to_rows, oy), im.sample_image_offsets(rows, to_rows, oy))):
            assert library is not None and np.array_equal(python, library), what
        assert np.array_equal(got % cols, np.broadcast_to(sample_offsets(cols, to_cols, ox), got.shape)), what
        assert np.array_equal(got // cols, np.broadcast_to(sample_offsets(rows, to_rows, oy)[:, None], got.shape)), what
        assert_same(restate_sample(px, to_rows, to_cols, offset), got.astype(np.uint16)[..., None], what)


def test_offsets_that_leave_the_frame_are_declined():
    import imagemagick_amd as im
    im.load()
    assert im.sample_image_offsets(64, 16, 100.5) is None
    assert im.sample_image_offsets(64, 16, 250.0) is None
    assert im.sample_image_offsets(64, 16, 100.0) is not None
    assert im.sample_image_offsets(64, 16, 0.0) is not None
