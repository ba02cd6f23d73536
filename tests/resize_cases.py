"""The case tables of tests/test_gpu_resize_filters.py and the window formula of the reference's
HorizontalFilter / VerticalFilter (resize.c:3364-3380, :3418-3443) they are checked with.  Nothing here
looks inside the library: the tap count of a case follows from the filter's support and the two sizes."""
import numpy as np

EPSILON = 1.0e-12                    # MagickEpsilon

SOURCE_ROWS, SOURCE_COLUMNS = 23, 37


def filter_names():
    """Every named filter the library builds: all but Undefined and the cylindrical Jinc."""
    from imagemagick_amd import _lib
    return [n for n in _lib.FILTERS if n not in ("undefined", "jinc")]


def windows(support, source, destination):
    """(start, count) of every destination sample's window along one axis."""
    factor = float(destination) * (1.0 / float(source))           # resize.c:3804-3805
    scale = max(1.0 / factor + EPSILON, 1.0)
    support = scale * support
    if support < 0.5:
        support = 0.5
    out = []
    for x in range(destination):
        bisect = (x + 0.5) / factor + EPSILON
        start = int(max(bisect - support + 0.5, 0.0))
        stop = int(min(bisect + support + 0.5, float(source)))
        out.append((start, max(stop - start, 0)))
    return out


def max_taps(support, source, destination):
    return max(count for _, count in windows(support, source, destination))


# The horizontal kernel is chosen by the largest window of the pass (resize_pass_plan.hpp, horizontal_launch): a tile of
# converted samples with 4, 6, 7 or 8 taps a lane, or the plain tile with 8, 16, 32 or any number.
TAP_CLASSES = ["<=4", "5-6", "7", "8", "9-16", "17-32", ">32"]


def tap_class(taps):
    for name, limit in zip(TAP_CLASSES, (4, 6, 7, 8, 16, 32)):
        if taps <= limit:
            return name
    return TAP_CLASSES[-1]


# (class, filter, source columns, target columns, largest window,
#  target rows that run the horizontal filter first (x factor > y factor), target rows that run it second)
# Source rows are always SOURCE_ROWS.
TAP_CASES = [
    ("<=4", "mitchell", 37, 85, 4, 29, 60),
    ("5-6", "lanczos", 37, 85, 6, 29, 60),
    ("7", "lanczos", 37, 37, 7, 19, 31),
    ("7", "magickernelsharp2013", 37, 30, 7, 11, 20),
    ("8", "sinc", 37, 85, 8, 29, 60),
    ("9-16", "magickernelsharp2021", 37, 85, 9, 29, 60),
    ("9-16", "lanczos", 37, 19, 12, 9, 14),
    ("17-32", "lanczos", 37, 13, 18, 7, 12),
    ("17-32", "magickernelsharp2021", 37, 13, 26, 7, 12),
    (">32", "lanczos", 300, 33, 55, 2, 5),
]

# A Point reduction whose 256-column tile spans 5120 source columns: as doubles, four channels, 160 KiB —
# past the 150 KiB the converted-tile form may use, so the plain 8-tap kernel takes it.
WIDE_POINT = ("point", (3, 5200), (3, 260))
CONVERTED_TILE_LIMIT = 150 * 1024
DEGENERATE_COLUMNS = [(1, 40), (40, 1), (2, 9)]

def verify_tap_cases(support_of):
    """The largest window of every case, recomputed from the filter's support (support_of(name): the library's
    MhGetResizeFilterSupport) with the reference's formula, is the one the table states; the table reaches all
    seven classes, each case has its two orders of the filters, and the wide Point reduction has one or two
    taps and a 256-column tile too wide for the converted form at four channels."""
    reached = set()
    for cls, filt, source, target, taps, rows_first, rows_second in TAP_CASES:
        got = max_taps(support_of(filt), source, target)
        assert got == taps and tap_class(got) == cls, (filt, source, target, got)
        reached.add(cls)
        x_factor = target * (1.0 / source)
        assert x_factor > rows_first * (1.0 / SOURCE_ROWS), (filt, source, target, rows_first)
        assert not x_factor > rows_second * (1.0 / SOURCE_ROWS), (filt, source, target, rows_second)
    assert reached == set(TAP_CLASSES), reached
    filt, (rows, cols), (to_rows, to_cols) = WIDE_POINT
    w = windows(support_of(filt), cols, to_cols)
    assert max(count for _, count in w) <= 2
    span = max(s + c for s, c in w[:256]) - min(s for s, _ in w[:256])
    assert span * 4 * 8 > CONVERTED_TILE_LIMIT, span


# layout -> (channels, has_alpha)
LAYOUTS = {"gray": (1, False), "two plain": (2, False), "gray+alpha": (2, True), "rgb": (3, False),
           "four plain": (4, False), "rgba": (4, True)}

# B1: (columns, rows) an enlargement, a reduction, one of each — and two enlargements whose y factor is the larger
# one, so that the vertical filter runs first and FAST may take a one-launch form: x2 across (the streaming form's
# geometry) and x2.3 across (the matrix-pipe form's)
FILTER_TARGETS = [(85, 51), (13, 9), (74, 9), (74, 58), (85, 60)]

# Channel masks: layout -> [(ParseChannelOption string, MhImage channel_mask, stored offsets that carry Copy)].
# A strict subset of the colour channels stays updated; the last entry of a layout with alpha masks alpha out alone.
MASK_CASES = {
    "gray+alpha": [("R", 0x1, (1,)), ("A", 0x10, (0,))],
    "rgb": [("R", 0x1, (1, 2)), ("RB", 0x5, (1,))],
    "rgba": [("G", 0x2, (0, 2, 3)), ("RB", 0x5, (1, 3)), ("A", 0x10, (0, 1, 2)), ("RGB", 0x7, (3,))],
}
MASK_TARGETS = [(74, 58), (13, 9)]          # x2 across and x2.52 down (FAST: a one-launch candidate), a reduction

# B4: wide supports through FAST's one-launch forms; (rows, columns) and the horizontal factors
WIDE_FILTERS = ["sinc", "magickernelsharp2021", "magickernelsharp2013"]
WIDE_SHAPES = [(37, 58), (64, 130), (29, 33)]
WIDE_FACTORS = [2.0, 3.0, 4.0, 2.3]
ONE_LAUNCH_KERNELS = {"resize_stream", "resize_stream_careful", "resize_mfma", "resize_vertical", "resize_horizontal"}


def wide_target(shape, factor):
    """(columns, rows): `factor` across, a little more down, so that the vertical filter runs first."""
    rows, columns = shape
    return int(round(columns * factor)), int(rows * factor) + 3


def source_frame(rows, columns, channels, dtype, alpha, seed=0):
    """Noise over the whole Quantum range (non-integral on float frames); with alpha, the first fifth of
    the columns transparent and the upper half of the rows opaque elsewhere."""
    rng = np.random.default_rng(7741 + seed + 1000 * rows + columns + 7 * channels)
    a = rng.integers(0, 65536, (rows, columns, channels), dtype=np.uint16)
    if dtype == np.float32:
        a = np.minimum(a.astype(np.float32) + rng.random((rows, columns, channels), dtype=np.float32),
                       np.float32(65535.0))
    if alpha:
        a[: rows // 2, :, channels - 1] = 65535
        a[:, : columns // 5, channels - 1] = 0
    return np.ascontiguousarray(a)
