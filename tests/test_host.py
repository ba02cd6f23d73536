"""CPU tests (`-m "not gpu"`) of the product's host side: the C-ABI library
loads and exports every symbol include/magickhip.h declares, and the host-side
builders (kernels, resize filters, LUTs — no device work) reproduce the
reference's tables bit for bit.  No compute entry point is exercised beyond its
argument/gate handling, which must fail loudly (never fall back to a CPU
implementation) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import gpu_available
from oracle import restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(GOLDEN, "reference_vectors.npz"))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "magickhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#\s*define[^\n]*", "", text)
    return sorted(set(re.findall(r"MH_API[^;(]*?\b(\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol(im):
    from imagemagick_amd import _lib
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, "libmagickhip.so lacks %s" % missing
    bound = {p[0] for p in _lib.PROTOTYPES}
    assert set(names) == bound, "binding and header disagree: %s" % (set(names) ^ bound)


def test_no_torch_or_cxx_types_in_the_abi():
    text = open(os.path.join(ROOT, "include", "magickhip.h")).read()
    assert 'extern "C"' in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "torch" not in text and "std::" not in text and "hipStream_t" not in text


def test_binding_names_every_operator_kind_of_the_header():
    """Every `MH_OP_<NAME> = <n>` of include/magickhip.h is `<name without underscores, lower case>: <n>` in
    the binding's OPERATORS, and OPERATORS holds nothing else: the part of keeping the kinds in one place
    that the library's own build-time check of its operator table cannot see."""
    from imagemagick_amd import _lib
    text = open(os.path.join(ROOT, "include", "magickhip.h")).read()
    declared = {name.replace("_", "").lower(): int(value)
                for name, value in re.findall(r"\bMH_OP_(\w+)\s*=\s*(\d+)", text)}
    assert len(declared) >= 27 and sorted(declared.values()) == list(range(1, len(declared) + 1))
    assert _lib.OPERATORS == declared


def test_operators_fail_loudly_without_a_device(im):
    if gpu_available():
        pytest.skip("a GPU is present")
    px = np.zeros((8, 8, 4), np.uint16)
    with pytest.raises(im.MagickHipError) as e:
        im.blur_image(im.Image(px), 0.0, 2.0)
    assert e.value.status in (2, 6)           # MH_NO_DEVICE / MH_DISABLED: the caller runs its CPU path
    assert im.device_count() == 0


def test_bad_arguments_are_rejected(im):
    from imagemagick_amd import _lib
    lib = _lib.load()
    d = _lib.MhImage()
    lib.MhInitImage(ctypes.byref(d), None, 4, 4, 4, 1, 0, 0)
    assert lib.MagickHipBlurImage(ctypes.byref(d), ctypes.byref(d), 0.0, 1.0) != 0     # NULL pixels
    assert lib.MagickHipBlurImage(None, None, 0.0, 1.0) != 0
    assert lib.MhGetLastError() is not None
    assert lib.MhAcquireKernelInfo(b"NoSuchKernel:3") is None or not lib.MhAcquireKernelInfo(b"NoSuchKernel:3")


def test_init_image_traits(im):
    """InitializePixelChannelMap + default channel mask, pixel.c:6132-6205, :6338-6393."""
    from imagemagick_amd import _lib
    lib = _lib.load()
    d = _lib.MhImage()
    lib.MhInitImage(ctypes.byref(d), None, 5, 7, 4, 1, 0, 0)
    assert list(d.channel_traits) == [6, 6, 6, 2] and d.alpha_offset == 3     # Update|Blend x3, Update
    lib.MhInitImage(ctypes.byref(d), None, 5, 7, 3, 0, 0, 0)
    assert list(d.channel_traits)[:3] == [2, 2, 2] and d.alpha_offset == -1


# ---------------------------------------------------------------- kernel builder
@pytest.mark.parametrize("spec", ["blur:0x2", "blur:0x10", "blur:0x0.5", "blur:4x1.5", "blur:0x10+90",
                                  "Disk:15", "Disk:2.5", "Gaussian:0x1.5", "3x3: 1,-,1 2,4,2 1,nan,3"])
def test_kernel_builder_matches_reference(im, vectors, spec):
    values, x, y, _ = im.kernel_to_numpy(spec)
    want = vectors["kernel|" + spec]
    assert values.shape == want.shape, spec
    assert np.array_equal(np.isnan(values), np.isnan(want)), spec
    assert np.array_equal(np.nan_to_num(values), np.nan_to_num(want)), "%s: values differ" % spec
    assert [x, y] == list(vectors["kernel_origin|" + spec]), spec


def _kernel_list_names(vectors):
    return sorted({k.split("|")[1] for k in vectors.files if k.startswith("kernellist|")})


def test_kernel_lists_match_reference(im, vectors):
    """Every kernel of the hit-and-miss sets (Edges, Corners, Diagonals, LineEnds, LineJunctions,
    Ridges, ConvexHull, Skeleton, ThinSE), FreiChen, the larger Laplacians and the rotation /
    mirror expansion flags (>, @, <): values, NaN cells and origins as AcquireKernelInfo builds
    them (morphology.c:485-560, :1748-2087, :2332-2450, :4258-4429)."""
    names = _kernel_list_names(vectors)
    assert len(names) >= 40
    for spec in names:
        count = int(vectors["kernellist|%s|count" % spec][0])
        assert im.kernel_to_numpy(spec)[3] == count, spec
        for i in range(count):
            values, x, y, _ = im.kernel_to_numpy(spec, i)
            want = vectors["kernellist|%s|%d" % (spec, i)]
            assert values.shape == want.shape, (spec, i)
            assert np.array_equal(np.isnan(values), np.isnan(want)), (spec, i)
            assert np.array_equal(np.nan_to_num(values), np.nan_to_num(want)), (spec, i)
            assert [x, y] == list(vectors["kernellist_origin|%s|%d" % (spec, i)]), (spec, i)


def test_kernel_builder_matches_oracle(im):
    for radius, sigma in ((0.0, 2.0), (0.0, 10.0), (0.0, 0.7), (6.0, 3.0)):
        values, x, y, count = im.kernel_to_numpy("blur:%.20gx%.20g;blur:%.20gx%.20g+90" %
                                                 (radius, sigma, radius, sigma))
        assert count == 2
        want = R.blur_kernel(radius, sigma)
        assert np.array_equal(values.ravel(), want) and x == (want.size - 1) // 2 and y == 0
        v2, x2, y2, _ = im.kernel_to_numpy("blur:%.20gx%.20g;blur:%.20gx%.20g+90" %
                                           (radius, sigma, radius, sigma), 1)
        assert v2.shape == (want.size, 1) and np.array_equal(v2.ravel(), want) and (x2, y2) == (0, x)


def test_outer_product_kernels_are_recognised(im):
    """Host logic of the FAST separated ConvolveImage: Gaussian / Square / hand-written outer
    products factor (and the factors reproduce the kernel to 1e-13 of its largest cell), kernels
    with holes, rings or asymmetric cells do not."""
    for spec in ("Gaussian:0x2", "Gaussian:0x10", "Gaussian:3x1.5", "Square:2", "Unity", "Sobel",
                 "5x3+1+2: 0.01,0.02,0.03,0.02,0.01 0.02,0.04,0.06,0.04,0.02 0.03,0.06,0.09,0.06,0.03"):
        values, _, _, _ = im.kernel_to_numpy(spec)
        factors = im.kernel_outer_product_factors(spec)
        assert factors is not None, spec
        row, column = factors
        assert row.shape == (values.shape[1],) and column.shape == (values.shape[0],)
        assert np.abs(np.outer(column, row) - values).max() <= 1e-13 * np.abs(values).max(), spec
    for spec in ("Disk:2.5", "Diamond:2", "Ring:1,2.5", "Laplacian:0", "LoG:0x2", "DoG:0,1,2",
                 "3x3: 0,1,0 1,-3,1 0,1,1", "3x3: 1,nan,1 1,1,1 1,1,1"):
        assert im.kernel_outer_product_factors(spec) is None, spec


def test_outer_product_plus_origin_cell_kernels_are_recognised(im):
    """Host logic of the EXACT separated ConvolveImage: SharpenImage's negated Gaussian whose centre
    carries the normalisation (effect.c:3640-3660) and EdgeImage's box of -1 with w*h-1 in the middle
    (effect.c:1530-1545) are an outer product + one cell; the factors never read the odd cell."""
    def spec_of(values):
        h, w = values.shape
        return "%dx%d: %s" % (w, h, " ".join(",".join("%.17g" % v for v in r) for r in values))

    x = np.arange(-3, 4, dtype=np.float64)
    gauss = -np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * 1.5 ** 2))
    sharpen = gauss.copy()
    sharpen[3, 3] = -2.0 * (gauss.sum() - gauss[3, 3])
    edge = -np.ones((5, 5))
    edge[2, 2] = 24.0
    wide = -np.outer([1.0, 2.0, 1.0], [1.0, 3.0, 5.0, 3.0, 1.0])
    wide[1, 2] += 40.0
    for values in (sharpen, edge, wide):
        got = im.kernel_outer_product_plus_delta(spec_of(values))
        assert got is not None
        kind, row, column, delta = got
        assert kind == 2 and delta != 0.0
        rebuilt = np.outer(column, row)
        rebuilt[values.shape[0] // 2, values.shape[1] // 2] += delta
        assert np.abs(rebuilt - values).max() <= 1e-13 * np.abs(values).max()
        assert im.kernel_outer_product_factors(spec_of(values)) is None
    # a plain outer product reports kind 1 and no delta
    kind, row, column, delta = im.kernel_outer_product_plus_delta("Gaussian:0x2")
    assert kind == 1 and delta == 0.0
    # two odd cells, an odd cell off the origin, NaN holes, kernels too small: no
    two = sharpen.copy(); two[0, 0] += 0.5
    off = gauss.copy(); off[1, 1] += 3.0
    for values in (two, off):
        assert im.kernel_outer_product_plus_delta(spec_of(values)) is None
    for spec in ("Disk:2.5", "Ring:1,2.5", "3x3: 1,nan,1 1,9,1 1,1,1", "1x3: 1,5,1"):
        got = im.kernel_outer_product_plus_delta(spec)
        assert got is None or got[0] == 1, spec


def test_integer_multiple_kernels_are_recognised(im):
    """Host logic of the exact-integer 2-D convolve (convolve2d_exact.hip): after `convolve:scale='!'`
    every flat shape kernel is one unit times 0/1 cells, integer kernels are small multiples, NaN
    cells count as no cell; Gaussians, LoG and kernels with a cell beyond 127 units are not."""
    for spec in ("Disk:15", "Disk:7.3", "Octagon:5", "Diamond:4", "Plus:3", "Ring:10,14", "Square:3", "Rectangle:8x4",
                 "7x5: 1,2,3,4,3,2,1 2,4,6,8,6,4,2 3,6,9,13,9,6,2 2,4,6,8,6,4,2 1,2,3,4,3,2,1",
                 "3x3: 1,nan,2 0,3,0 2,nan,1", "3x3: 2,3,2 3,2,3 2,3,2", "3x3: -1,-1,-1 -1,24.5,-1 -1,-1,-1"):
        values, _, _, _ = im.kernel_to_numpy(spec)
        for scale in (None, (1.0, 1)):
            got = im.kernel_integer_cells(spec, scale=scale)
            assert got is not None, (spec, scale)
            cells, unit = got
            assert cells.shape == values.shape and unit > 0.0 and np.abs(cells).max() <= 127
            assert (cells[np.isnan(values)] == 0).all()
            if scale is None:
                # cells * unit reproduces the kernel, and the unit is a cell or a simple fraction of one
                assert np.allclose(np.where(np.isnan(values), 0.0, values), cells * unit, rtol=1e-9, atol=0.0)
    cells, unit = im.kernel_integer_cells("Disk:15", scale=(1.0, 1))
    assert int(cells.sum()) == 709 and set(np.unique(cells)) == {0, 1} and abs(unit * 709.0 - 1.0) < 1e-12
    cells, unit = im.kernel_integer_cells("3x3: 2,3,2 3,2,3 2,3,2")
    assert unit == 1.0 and cells.min() == 2                       # the unit is half the smallest cell
    for spec in ("Gaussian:0x2", "LoG:0x2", "DoG:0,1,2", "3x3: 1,1,1 1,300,1 1,1,1", "3x3: 1,1,1 1,0.123456,1 1,1,1",
                 "3x3: nan,0,nan 0,0,0 nan,0,nan"):
        assert im.kernel_integer_cells(spec) is None, spec


def test_optimal_kernel_width(im):
    from imagemagick_amd import _lib
    lib = _lib.load()
    for sigma in (0.3, 0.5, 1.0, 2.0, 3.7, 10.0, 25.0):
        assert lib.MhGetOptimalKernelWidth1D(0.0, sigma) == R.optimal_kernel_width_1d(0.0, sigma)
    assert lib.MhGetOptimalKernelWidth1D(0.0, 10.0) == 79          # 79 taps on Q16
    assert lib.MhGetOptimalKernelWidth1D(0.0, 2.0) == 17
    assert lib.MhGetOptimalKernelWidth1D(2.2, 1.0) == 7


# ----------------------------------------------------------------- resize filter
FILTERS = ["Lanczos", "Mitchell", "Catrom", "Triangle", "Box", "Gaussian", "Hann", "Spline", "Cubic",
           "Hermite", "Lanczos2", "LanczosSharp", "Robidoux", "Sinc", "Hamming", "Blackman", "Quadratic"]


@pytest.mark.parametrize("name", FILTERS)
def test_resize_filter_matches_reference(im, vectors, name):
    from imagemagick_amd import _lib
    lib = _lib.load()
    f = lib.MhAcquireResizeFilter(_lib.FILTERS[name.lower()], 0)
    assert f
    try:
        assert lib.MhGetResizeFilterSupport(f) == vectors["filter_support|" + name][0]
        got = np.array([lib.MhGetResizeFilterWeight(f, float(x)) for x in vectors["filter_xs"]])
        want = vectors["filter|" + name]
        # sin/cos-based windows go through libm on both sides: identical here, 2 ULP allowed
        assert np.allclose(got, want, rtol=0, atol=4.5e-16), "%s: max diff %g" % (name, np.abs(got - want).max())
        if name in ("Lanczos", "Mitchell", "Catrom", "Triangle", "Box", "Spline", "Cubic", "Hermite",
                    "Lanczos2", "LanczosSharp", "Robidoux", "Quadratic"):
            assert np.array_equal(got, want), name          # polynomial filters: bit-identical
    finally:
        lib.MhDestroyResizeFilter(f)


@pytest.fixture(scope="module")
def filter_vectors():
    return np.load(os.path.join(GOLDEN, "resize_filter_vectors.npz"))


def _all_filter_names():
    from imagemagick_amd import _lib
    return [n for n in _lib.FILTERS if n not in ("undefined", "jinc")]


# Weighting and windowing functions that are polynomials in x (resize.c: Box, Triangle, CubicBC, Quadratic,
# Lagrange, CubicSpline, MagicKernelSharp2013 / 2021): no libm call, the weights are bit-identical everywhere.
POLYNOMIAL_FILTERS = {"point", "box", "triangle", "hermite", "quadratic", "cubic", "catrom", "mitchell", "lagrange",
                      "robidoux", "robidouxsharp", "spline", "cubicspline", "magickernelsharp2013", "magickernelsharp2021"}
# SincFast is a polynomial up to x = 4 and sin(pi x)/(pi x) beyond (resize.c:493-587); windowed by itself, by
# Box, Welch, a cubic or a triangle, such a filter calls no libm function while |x|/blur <= 4.  The sharpened
# variants shrink x by blur >= 0.9549: |x| <= 3.75 stays on the polynomial for every one of them.
SINCFAST_FILTERS = {"sincfast", "lanczos", "lanczossharp", "lanczos2", "lanczos2sharp", "lanczosradius", "welch",
                    "parzen", "bartlett"}
# sin, cos, exp, sqrt or the Bessel series on every abscissa: within the module's 2 ULP of a weight of 1
LIBM_FILTERS = {"hann", "hamming", "blackman", "gaussian", "sinc", "kaiser", "bohman", "cosine"}


def test_resize_filter_fixture_covers_every_filter_on_a_grid_that_reaches_its_support(filter_vectors):
    names = _all_filter_names()
    assert list(filter_vectors["names"]) == names and len(names) == 32
    assert POLYNOMIAL_FILTERS | SINCFAST_FILTERS | LIBM_FILTERS == set(names)
    assert not (POLYNOMIAL_FILTERS & SINCFAST_FILTERS or POLYNOMIAL_FILTERS & LIBM_FILTERS or SINCFAST_FILTERS & LIBM_FILTERS)
    xs = filter_vectors["xs"]
    assert xs.min() == -5.25 and xs.max() == 5.25 and np.all(np.diff(xs) > 0.0)
    for half in np.arange(-10, 11) / 2.0:
        assert half in xs
    for name in names:
        support = filter_vectors["support|" + name][0]
        assert 0.0 <= support < 5.25 and support in xs and -support in xs, name


@pytest.mark.parametrize("name", _all_filter_names())
def test_every_resize_filter_matches_reference(im, filter_vectors, name):
    """Support and weights of every named filter the library builds (kFilters, kMapping and evaluate of
    resize_filter.cpp) against AcquireResizeFilter / GetResizeFilterWeight of the compiled reference, on a
    grid that holds 0, the half-integers, every filter's support and the doubles on either side of it,
    and reaches past the widest support.  (Kaiser's window takes sqrt of a negative number beyond its
    support; the Bessel series of a NaN is 1 on both sides, so no weight is a NaN.)"""
    from imagemagick_amd import _lib
    lib = _lib.load()
    f = lib.MhAcquireResizeFilter(_lib.FILTERS[name], 0)
    assert f, name
    try:
        assert lib.MhGetResizeFilterSupport(f) == filter_vectors["support|" + name][0], name
        xs = filter_vectors["xs"]
        got = np.array([lib.MhGetResizeFilterWeight(f, float(x)) for x in xs])
    finally:
        lib.MhDestroyResizeFilter(f)
    want = filter_vectors["weights|" + name]
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern differs" % name
    finite = ~np.isnan(want)
    diff = np.abs(got[finite] - want[finite])
    print("%s: max |diff| %g, %d of %d weights differ" % (name, diff.max(), int((diff > 0).sum()), diff.size))
    assert diff.max() <= 4.5e-16, "%s: max diff %g" % (name, diff.max())
    if name in POLYNOMIAL_FILTERS:
        bitwise = finite
    elif name in SINCFAST_FILTERS:
        bitwise = finite & (np.abs(xs) <= 3.75)
    else:
        bitwise = np.zeros_like(finite)
    assert np.array_equal(got[bitwise].view(np.uint64), want[bitwise].view(np.uint64)), \
        "%s: %d weights of the polynomial range differ" % (name, int((got[bitwise] != want[bitwise]).sum()))


def test_jinc_and_out_of_range_filter_types_are_declined(im):
    """Jinc is cylindrical-only (resize.c:841-877 maps it to itself, and ResizeImage never reaches it with an
    orthogonal meaning here): MhAcquireResizeFilter returns null for it, for Undefined and for every type
    outside the enumeration, and says why."""
    from imagemagick_amd import _lib
    lib = _lib.load()
    sentinel = max(_lib.FILTERS.values()) + 1
    for filter_type in (_lib.FILTERS["jinc"], _lib.FILTERS["undefined"], -1, -1000, sentinel, sentinel + 1, 1 << 20):
        assert not lib.MhAcquireResizeFilter(filter_type, 0), filter_type
    assert not lib.MhAcquireResizeFilter(_lib.FILTERS["jinc"], 0)
    assert b"Jinc" in lib.MhGetLastError()


def test_resize_tap_case_table_reaches_every_class(im):
    """tests/resize_cases.py, the table of the GPU resize suite: checked here too, where no device is needed."""
    import resize_cases
    from imagemagick_amd import _lib
    lib = _lib.load()

    def support_of(name):
        f = lib.MhAcquireResizeFilter(_lib.FILTERS[name], 0)
        assert f, name
        try:
            return lib.MhGetResizeFilterSupport(f)
        finally:
            lib.MhDestroyResizeFilter(f)

    resize_cases.verify_tap_cases(support_of)


# -------------------------------------------------------------------- LUT builders
@pytest.mark.parametrize("hdri", [False, True])
def test_lut_builders_reproduce_the_operators(im, vectors, hdri):
    tag = "hdri" if hdri else "q16"
    px = vectors[tag + "_smooth_in"]
    rows, cols, ch = px.shape
    n = rows * cols
    quantum = 1 if hdri else 0
    inten = R.pixel_intensity(px)
    idx = R.scale_quantum_to_map(R.clamp_to_quantum(inten, hdri), hdri)
    hist = np.zeros((65536, ch), dtype=np.uint64)
    for c in range(ch):
        hist[:, c] = np.bincount(idx.ravel(), minlength=65536)
    own = R.scale_quantum_to_map(px, hdri)

    def apply(lut, mask):
        out = px.copy()
        for c in range(ch):
            if (mask >> c) & 1:
                out[:, :, c] = R.clamp_to_quantum(lut[own[:, :, c], c], hdri)
        return out

    lut, mask = im.contrast_stretch_lut(hist, cols, rows, 0.02 * n, n - 0.01 * n, quantum)
    assert np.array_equal(apply(lut, mask), vectors[tag + "_smooth_cstretch"])
    lut, mask = im.equalize_lut(hist, quantum)
    assert np.array_equal(apply(lut, mask), vectors[tag + "_smooth_equalize"])


def test_default_precision_is_fast_and_the_environment_selects_exact():
    """What an unchanged MagickCore caller gets is MH_PRECISION_FAST (within one level / one float ULP:
    the drop-in's contract and bench.py's `value`); MAGICK_HIP_PRECISION=exact selects the bit-identical
    mode.  A fresh process each: the library reads its environment once."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import imagemagick_amd as im; im.load(); print('precision', im.get_precision())"
    for value, want in ((None, 1), ("exact", 0), ("fast", 1)):
        env = {k: v for k, v in os.environ.items() if k != "MAGICK_HIP_PRECISION"}
        if value is not None:
            env["MAGICK_HIP_PRECISION"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=300)
        assert "precision %d" % want in out.stdout, (value, out.stdout[-2000:])
