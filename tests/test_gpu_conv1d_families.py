"""Every kernel family of convolve.hip and convolve_folded.hip at the smallest frames where its tile arithmetic can go
wrong, against the compiled reference.

Route: MorphologyImage(Convolve) with a K x 1 or 1 x K kernel goes straight to launch_conv1d (operators.cpp,
primitive()), past the fused blurs.  The tap counts sit on both sides of every switch of the dispatch code: 16 taps
(blocked / plain -> triangular), 24 (FAST blocked -> triangular), the strip sizes at which the fp64 column pass goes
from eight staged waves to four to the unstaged kernel (97 | 98, 129 | 130 taps for 8-byte pixels; 17 | 18, 49 | 50
for 16-byte ones), and launch_folded's <R,U> pairs (3, 5, 9 taps a row; 3, 5, 25 a column).

Frames, as (rows, columns): the smallest; one where every read is clamped; a second tile column with a ragged tile
row; the second 128-row tile of the eight-wave column pass; a second 512-column row segment (for float RGBA also the
whole-segment store through LDS); a second segment of the FAST kernels' sixteen outputs a lane.

Contract (conftest.assert_parity): EXACT and float Quantum bit-identical, FAST within one level."""
import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
SHAPES = [(1, 1), (5, 7), (67, 131), (131, 67), (5, 515)]
FAST_SHAPES = SHAPES + [(5, 1027)]
# (channels, alpha-weighted)
LAYOUTS = [(1, False), (2, True), (3, False), (4, True), (4, False)]
RGBA = [(4, True)]


def taps(n, negative=False):
    """n taps that sum to one, not quite symmetric; negative: one of them below zero."""
    w = [(i + 1.0) * (n - i) + (i % 3) for i in range(n)]
    if negative:
        w[n // 3] = -w[n // 3]
    total = sum(abs(v) for v in w)
    return ",".join("%.17g" % (v / total) for v in w)


def kernel_1d(n, vertical, negative=False):
    return ("1x%d: " % n if vertical else "%dx1: " % n) + taps(n, negative)


def frame(shape, channels, alpha, dtype, seed):
    px = make_pixels(shape[0], shape[1], channels, dtype, seed=seed + 31 * channels + shape[1])
    if alpha and shape[1] > 40:                      # small and zero alpha where the frame has room for it
        px[:, 8:20, channels - 1] = (np.arange(12) % 4).astype(px.dtype)
        px[:, 30:36, channels - 1] = 0
    return px


def reference(refmod, px, alpha, kernel, bias=0.0, mask=None, scale=False):
    def run(pixels):
        ref = refmod.RefImage(pixels)
        if mask:
            ref.set_channel_mask(mask)
        if scale:
            ref.set_artifact("convolve:scale", "!")
        if bias:
            ref.set_artifact("convolve:bias", "%.17g" % bias)
        return ref.morphology("Convolve", 1, kernel).numpy()
    if px.shape[2] in (2, 4) and not alpha:          # channels without an alpha: each one on its own
        return np.concatenate([run(px[:, :, c].copy()).reshape(px.shape[0], px.shape[1], 1)
                               for c in range(px.shape[2])], axis=2)
    return run(px).reshape(px.shape)


def same(got, want, exact, what):
    if want.dtype == np.float32:
        equal = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert equal.all(), "%s: %d float samples differ" % (what, int((~equal).sum()))
    else:
        assert_parity(got, want, exact, what)


def run_1d(im, refmod, dtype, counts, layouts, shapes, exact=True, negative=False, bias=0.0, mask=None, copy=(),
           audit=False):
    """Both passes of every tap count on every frame and layout; the pass's own ProfileScope label and not the
    other's (a 1 x 1 kernel is a column kernel to primitive()).  audit: the row pass is followed by the alpha audit."""
    import bench
    for shape in shapes:
        for channels, alpha in layouts:
            px = frame(shape, channels, alpha, dtype, seed=len(counts))
            dev = im.Image(to_device(px), has_alpha=alpha, copy_channels=copy)
            for n in counts:
                for vertical in (False, True):
                    kernel = kernel_1d(n, vertical, negative)
                    holder = {}
                    launched = set(bench.kernel_profile(
                        im, lambda: holder.update(out=im.morphology_image(dev, "Convolve", 1, kernel, bias=bias)), 1))
                    what = "%d taps %s, %s %s c%d alpha=%s bias %g mask %s (%s)" % (
                        n, "column" if vertical else "row", shape, np.dtype(dtype).name, channels, alpha, bias, mask,
                        " ".join(sorted(launched)))
                    column = vertical or n == 1
                    assert ("conv_column" in launched) == column and ("conv_row" in launched) == (not column), what
                    assert ("conv_row_alpha_audit" in launched) == (audit and not column), what
                    same(holder["out"].numpy().reshape(px.shape), reference(refmod, px, alpha, kernel, bias, mask),
                         exact, what)


# ------------------------------------------------------------------ Q16, EXACT
@pytest.mark.parametrize("n", [1, 3, 15])
def test_q16_exact_blocked(im, refmod, n):
    run_1d(im, refmod, Q16, [n], LAYOUTS, SHAPES)


def test_q16_exact_triangular_tie(im, refmod):
    run_1d(im, refmod, Q16, [16], LAYOUTS, SHAPES)


@pytest.mark.parametrize("n", [97, 98, 129, 130])
def test_q16_exact_column_staging_switches(im, refmod, n):
    """8-wave staged | 4-wave staged | unstaged column pass of RGBA Q16 (8-byte pixels)."""
    run_1d(im, refmod, Q16, [n], RGBA, SHAPES)


def test_q16_exact_triangular_exact64(im, refmod):
    run_1d(im, refmod, Q16, [17], LAYOUTS, SHAPES, negative=True)
    run_1d(im, refmod, Q16, [17], LAYOUTS, SHAPES, bias=0.25)


# ------------------------------------------------------------------ Q16, FAST
def fast(im, call):
    im.set_precision(im.PRECISION_FAST)
    try:
        call()
    finally:
        im.set_precision(im.PRECISION_EXACT)


@pytest.mark.parametrize("n", [3, 23, 24, 79])
def test_q16_fast_vector_kernels(im, refmod, n):
    """Blocked Fast32 up to 23 taps, triangular from 24: one channel, three under a channel mask (the matrix
    path declines a Copy channel), and gray+alpha, whose FAST row pass is followed by the alpha audit."""
    fast(im, lambda: run_1d(im, refmod, Q16, [n], [(1, False)], FAST_SHAPES, exact=False))
    fast(im, lambda: run_1d(im, refmod, Q16, [n], [(2, True)], FAST_SHAPES, exact=False, audit=True))
    fast(im, lambda: run_1d(im, refmod, Q16, [n], [(3, False)], FAST_SHAPES, exact=False, mask="RG", copy=(2,)))


@pytest.mark.parametrize("sigma", [1.0, 4.0])
def test_q16_fast_gray_alpha_blur(im, refmod, sigma):
    """BlurImage on gray+alpha in FAST mode: both passes on these kernels.  (Its row pass feeds the column pass and
    therefore runs EXACT, operators.cpp primitive(): the alpha audit belongs to a FAST row pass whose result leaves
    the operator, test_q16_fast_vector_kernels.)"""
    import bench
    for shape in FAST_SHAPES:
        px = frame(shape, 2, True, Q16, seed=5)
        dev = im.Image(to_device(px), has_alpha=True)
        holder = {}

        def call():
            holder["launched"] = set(bench.kernel_profile(im, lambda: holder.update(out=im.blur_image(dev, 0.0, sigma)), 1))
        fast(im, call)
        what = "fast gray+alpha blur 0x%g %s (%s)" % (sigma, shape, " ".join(sorted(holder["launched"])))
        assert {"conv_row", "conv_column"} <= holder["launched"], what
        assert_parity(holder["out"].numpy().reshape(px.shape), refmod.RefImage(px).blur(0.0, sigma).numpy().reshape(px.shape),
                      False, what)


# ------------------------------------------------------------------ float Quantum
def test_float_triangular_tie(im, refmod):
    run_1d(im, refmod, HDRI, [16], LAYOUTS, SHAPES)


@pytest.mark.parametrize("n", [17, 18, 49, 50])
def test_float_column_staging_switches(im, refmod, n):
    """The staging switches for 16-byte pixels, and (5,515): the whole-segment store of the row pass through LDS."""
    run_1d(im, refmod, HDRI, [n], RGBA, SHAPES)


@pytest.mark.parametrize("n", [3, 15, 17])
def test_float_plain_kernels(im, refmod, n):
    run_1d(im, refmod, HDRI, [n], LAYOUTS, SHAPES, bias=0.25)
    run_1d(im, refmod, HDRI, [n], LAYOUTS, SHAPES, negative=True)


# ------------------------------------------------------------------ separable 2-D convolve
def outer_product(width, height):
    """A width x height kernel that is column x row, small integers (normalised by convolve:scale='!')."""
    row = [1 + min(i, width - 1 - i) for i in range(width)]
    column = [1 + min(i, height - 1 - i) + (i % 2) for i in range(height)]
    return "%dx%d: " % (width, height) + " ".join(",".join("%d" % (c * r) for r in row) for c in column)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("folded", [True, False])
@pytest.mark.parametrize("size", [(3, 3), (3, 9), (9, 3), (5, 7), (9, 25), (17, 5)])
def test_separable_passes(im, refmod, size, folded, dtype, options):
    """Every <R,U> pair of launch_folded; with the fold off, launch_conv1d_sums64: the plain Fma64 kernels below 16
    taps, the triangular ones from 16.  (A kernel of fewer than 25 cells, 3 x 3, stays on the generic 2-D kernel,
    operators.cpp: the <2,2> passes are reached by 3 x 9 and 9 x 3.)"""
    import bench
    options.set("MAGICKHIP_NO_EXACT_2D", "1")
    if not folded:
        options.set("MAGICKHIP_NO_SEPARABLE_FOLD", "1")
    kernel = outer_product(*size)
    for shape in SHAPES:
        for channels, alpha in LAYOUTS:
            px = frame(shape, channels, alpha, dtype, seed=size[0])
            dev = im.Image(to_device(px), has_alpha=alpha)
            holder = {}
            launched = set(bench.kernel_profile(
                im, lambda: holder.update(out=im.morphology_image(dev, "Convolve", 1, kernel, scale=(1.0, 1))), 1))
            what = "%s %s %s c%d alpha=%s folded=%s (%s)" % (kernel[:6], shape, np.dtype(dtype).name, channels, alpha,
                                                           folded, " ".join(sorted(launched)))
            if size[0] * size[1] < 25:
                assert not any(k.startswith(("separable", "conv_")) for k in launched), what
            elif folded:
                assert launched == {"separable_row_sums", "separable_column_finish", "separable_settle"}, what
            else:
                assert {"conv_row", "conv_column", "separable_finish"} <= launched, what
            same(holder["out"].numpy().reshape(px.shape), reference(refmod, px, alpha, kernel, scale=True), True, what)
