"""ResizeImage on the device against the compiled reference (RefImage.resize): every named filter, every
tap-count class of the two-pass kernels on every layout, channel masks, and the wide-support filters through
FAST's one-launch forms.  EXACT is bit-identical on both Quantum types; FAST is within one Quantum level or
one float ULP (a float result below 1e-9 of the largest sample is the residue of a cancellation and has no
last place: DESIGN.md section 2).  The frames are tiny on purpose; tests/resize_cases.py holds the tables."""
import numpy as np
import pytest

from conftest import to_device, assert_parity
from resize_cases import (DEGENERATE_COLUMNS, FILTER_TARGETS, LAYOUTS, MASK_CASES, MASK_TARGETS, ONE_LAUNCH_KERNELS,
                          SOURCE_COLUMNS, SOURCE_ROWS, TAP_CASES, WIDE_FACTORS, WIDE_FILTERS, WIDE_POINT, WIDE_SHAPES,
                          filter_names, source_frame, verify_tap_cases, wide_target)

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
TWO_PASSES = {"resize_vertical", "resize_horizontal"}
_REFERENCE = {}                    # computed once, shared by the precision modes and the routing switches


def reference(refmod, key, px, alpha, target, filt, mask=None):
    """RefImage.resize of px to target = (columns, rows).  A frame of 2 or 4 plain channels is that many gray
    frames to the reference (under the default channel mask it filters every channel alike)."""
    key = key + (px.dtype.name, alpha, target, filt, mask)
    if key not in _REFERENCE:
        cols, rows = target
        if alpha or px.shape[2] in (1, 3):
            image = refmod.RefImage(px)
            if mask is not None:
                image.set_channel_mask(mask)
            want = image.resize(cols, rows, filt).numpy()
        else:
            assert mask is None
            want = np.concatenate([refmod.RefImage(px[:, :, c].copy()).resize(cols, rows, filt).numpy()
                                   .reshape(rows, cols, 1) for c in range(px.shape[2])], axis=2)
        want.setflags(write=False)
        _REFERENCE[key] = want
    return _REFERENCE[key]


def resize(im, px, alpha, target, filt, exact, **kw):
    """(pixels, names of the kernels launched)."""
    import bench
    image = im.Image(to_device(px), has_alpha=alpha, precision=im.PRECISION_EXACT if exact else im.PRECISION_FAST, **kw)
    holder = {}
    launched = set(bench.kernel_profile(im, lambda: holder.update(out=im.resize_image(image, target[0], target[1], filt)), 1))
    return holder["out"].numpy(), launched


def check(got, want, px, exact, what):
    residue = 0.0
    if not exact and px.dtype == HDRI:
        residue = 1.0e-9 * float(np.abs(px).max())
    assert_parity(got, want, exact, what, max_ulp=0 if exact else 1, residue=residue)


def support_of(name):
    from imagemagick_amd import _lib
    lib = _lib.load()
    f = lib.MhAcquireResizeFilter(_lib.FILTERS[name], 0)
    assert f, name
    try:
        return lib.MhGetResizeFilterSupport(f)
    finally:
        lib.MhDestroyResizeFilter(f)


# ------------------------------------------------------------------------------ B1: every filter
@pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
@pytest.mark.parametrize("name", filter_names())
def test_every_filter_on_the_device(im, refmod, name, dtype):
    px = source_frame(SOURCE_ROWS, SOURCE_COLUMNS, 4, dtype, True)
    seen = set()
    for target in FILTER_TARGETS:
        want = reference(refmod, ("filters",), px, True, target, name)
        for exact in (True, False):
            got, launched = resize(im, px, True, target, name, exact)
            seen |= launched
            assert launched and launched <= ONE_LAUNCH_KERNELS, launched
            check(got, want, px, exact, "%s %dx%d -> %dx%d %s %s" % (
                name, SOURCE_COLUMNS, SOURCE_ROWS, target[0], target[1], px.dtype.name, "exact" if exact else "fast"))
    print("B1 %s %s launched %s" % (name, px.dtype.name, sorted(seen)))


def test_jinc_is_declined(im):
    px = source_frame(SOURCE_ROWS, SOURCE_COLUMNS, 4, Q16, True)
    with pytest.raises(im.MagickHipError) as e:
        im.resize_image(im.Image(to_device(px)), 85, 51, "jinc")
    assert e.value.status == 1                   # MH_UNSUPPORTED: the caller keeps its own path


# ------------------------------------------------- B2: tap-count classes of the two-pass kernels
def test_the_tap_case_table_reaches_every_class():
    """The largest window of every case, recomputed from the filter's support with the reference's formula,
    is the one the table states, and the table reaches all seven classes of the horizontal launcher."""
    verify_tap_cases(support_of)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", TAP_CASES, ids=["%s-%s-%dto%d" % c[:4] for c in TAP_CASES])
def test_tap_classes_on_every_layout(im, refmod, case, layout):
    """EXACT mode always runs the two passes; with the x factor above the y factor the horizontal filter
    reads the source frame, otherwise the vertical filter's result."""
    cls, filt, cols, to_cols, taps, rows_first, rows_second = case
    channels, alpha = LAYOUTS[layout]
    for dtype in (Q16, HDRI):
        px = source_frame(SOURCE_ROWS, cols, channels, dtype, alpha, seed=taps)
        for to_rows in (rows_first, rows_second):
            target = (to_cols, to_rows)
            want = reference(refmod, ("taps", layout), px, alpha, target, filt)
            got, launched = resize(im, px, alpha, target, filt, True)
            assert launched == TWO_PASSES, launched
            check(got, want, px, True, "%s taps, %s %s %dx%d -> %dx%d %s" % (
                cls, filt, layout, cols, SOURCE_ROWS, to_cols, to_rows, px.dtype.name))


@pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
def test_wide_point_reduction_takes_the_plain_tile(im, refmod, dtype):
    filt, (rows, cols), (to_rows, to_cols) = WIDE_POINT
    px = source_frame(rows, cols, 4, dtype, True)
    want = reference(refmod, ("point",), px, True, (to_cols, to_rows), filt)
    got, launched = resize(im, px, True, (to_cols, to_rows), filt, True)
    assert launched == TWO_PASSES, launched
    check(got, want, px, True, "Point %dx%d -> %dx%d %s" % (cols, rows, to_cols, to_rows, px.dtype.name))


@pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
@pytest.mark.parametrize("cols,to_cols", DEGENERATE_COLUMNS)
def test_degenerate_column_counts(im, refmod, cols, to_cols, dtype):
    px = source_frame(SOURCE_ROWS, cols, 4, dtype, True)
    for to_rows in (29, 17):
        want = reference(refmod, ("degenerate",), px, True, (to_cols, to_rows), "lanczos")
        got, launched = resize(im, px, True, (to_cols, to_rows), "lanczos", True)
        assert launched == TWO_PASSES, launched
        check(got, want, px, True, "Lanczos %dx%d -> %dx%d %s" % (cols, SOURCE_ROWS, to_cols, to_rows, px.dtype.name))


# ---------------------------------------------------------------------------- B3: channel masks
MASKED = [(layout,) + m for layout, masks in MASK_CASES.items() for m in masks]


@pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
@pytest.mark.parametrize("layout,mask,bits,copied", MASKED, ids=["%s-%s" % m[:2] for m in MASKED])
def test_channel_masks(im, refmod, layout, mask, bits, copied, dtype):
    """A channel the mask leaves out carries Copy: the nearest source sample, unweighted, in both filters
    (resize.c:3484-3485); the one-launch forms of FAST decline such a frame."""
    channels, alpha = LAYOUTS[layout]
    px = source_frame(SOURCE_ROWS, SOURCE_COLUMNS, channels, dtype, alpha, seed=3)
    seen = set()
    for target in MASK_TARGETS:
        want = reference(refmod, ("mask", layout), px, alpha, target, "lanczos", mask=mask)
        for exact in (True, False):
            got, launched = resize(im, px, alpha, target, "lanczos", exact, channel_mask=bits, copy_channels=copied)
            seen |= launched
            assert launched and launched <= ONE_LAUNCH_KERNELS, launched
            check(got, want, px, exact, "mask %s on %s -> %dx%d %s %s" % (
                mask, layout, target[0], target[1], px.dtype.name, "exact" if exact else "fast"))
    print("B3 %s %s %s launched %s" % (layout, mask, px.dtype.name, sorted(seen)))


# ------------------------------------- B4: wide supports through FAST's one-launch forms
@pytest.mark.parametrize("stream", [True, False], ids=["stream", "no-stream"])
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=["%dx%d" % s for s in WIDE_SHAPES])
@pytest.mark.parametrize("name", WIDE_FILTERS)
def test_wide_supports_through_the_one_launch_forms(im, refmod, options, name, shape, stream):
    """Sinc (support 4) and MagicKernelSharp2021 (4.5) put 8 to 10 source samples under an enlargement's
    window: more than the streaming form walks and more than any other test hands the matrix-pipe form.
    Whatever the router picks — either form or the two passes — keeps FAST's contract."""
    if not stream:
        options.set("MAGICKHIP_NO_RESIZE_STREAM", "1")
    rows, cols = shape
    seen = set()
    for alpha in (True, False):
        for dtype in (Q16, HDRI):
            px = source_frame(rows, cols, 4, dtype, alpha, seed=5)
            for factor in WIDE_FACTORS:
                target = wide_target(shape, factor)
                want = reference(refmod, ("wide",), px, alpha, target, name)
                got, launched = resize(im, px, alpha, target, name, False)
                seen |= launched
                assert launched and launched <= ONE_LAUNCH_KERNELS, launched
                assert stream or not launched & {"resize_stream", "resize_stream_careful"}, launched
                check(got, want, px, False, "%s %dx%d -> %dx%d %s %s" % (
                    name, cols, rows, target[0], target[1], "rgba" if alpha else "four plain", px.dtype.name))
    print("B4 %s %dx%d %s launched %s" % (name, cols, rows, "stream" if stream else "no-stream", sorted(seen)))
