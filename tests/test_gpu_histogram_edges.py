"""ContrastStretchImage / EqualizeImage (MagickCore/enhance.c:1544-1818, :2040-2280) on the device, through the C ABI,
against the compiled reference: the level-scan edges, the binning edges, the channel masks and the frame sizes at which
the launchers of histogram.hip change kernels.  Every comparison is bit for bit (float results as bit patterns), in
EXACT and in FAST: nothing on these paths reads the precision.  The one exception is the fused FAST sRGB -> Lab +
stretch (part I), whose Lab frame is within one level of the reference and whose stretch is exact on that frame.

Inputs hold no NaN (ScaleQuantumToMap casts the sample to unsigned int: undefined for NaN), +-Inf only where the bins
are per channel (an intensity of Inf - Inf is NaN), and every frame of three or more channels has a pixel with R != G
(the gray scan of ContrastStretchImage, enhance.c:1586-1588, then never declines by accident; part G declines on
purpose).  tests/test_histogram_edge_sizes.py keeps the sizes below tied to the constants of the kernels' sources.

The case that reaches each kernel:

  histogram_kernel, plain route             test_masks_on_large_frames[... period2]: per-channel bins at 2^20 pixels, no
                                            two neighbouring lanes agree; every frame below 2^20 pixels with random content
  histogram_kernel, leader election         test_masks_on_large_frames[... runs32] (32 equal pixels in a row: >= 16 lanes
                                            agree) and test_flat_frame_of_65_pixels (a last wave with invalid lanes)
  histogram_lds_kernel                      test_size_thresholds[1024x1024 ...], [17x61681 ...] under
                                            MAGICKHIP_NO_PACKED_HISTOGRAM
  histogram_packed_kernel<.., plain>        test_size_thresholds[1024x1024 ...], [17x61681 ...] with 3 and 4 channels
                                            (the three-term luma of an sRGB frame)
  histogram_packed_kernel<.., not plain>    the same with 1 and 2 channels (gray frames: the general intensity),
                                            test_packed_counter_carry, test_packed_more_workgroups_than_compute_units
  lut_chunk_sums_kernel / lut_scan_kernel   every case; the strict `>` of its black and white tests: test_tie_frame
  lut_stretch_map_kernel                    test_level_scan_edges, test_tie_frame, test_one_bin_frame under
                                            MAGICKHIP_NO_STRETCH_LEVELS
  stretch_apply_levels_kernel               the same tests without the option; its off-table black level (Q16 stores
                                            65536 as 0, float keeps 65536): the pairs (n, n) and (n+5, n)
  apply_lut_kernel                          test_level_scan_edges under MAGICKHIP_NO_STRETCH_LEVELS; EqualizeImage below
                                            2^20 pixels (test_size_thresholds[1023x1025 ...], test_binning_edges)
  apply_lut_shared_kernel                   test_size_thresholds[1024x1024 / 17x61681, Q16]: EqualizeImage, and the
                                            tabulated stretch
  equalize_cdf_apply_kernel, running counts test_float_equalize_group_counts[65535], test_float_equalize_flat_frames
                                            (level 12352 = 16 x 772: no bin of its group lies above its first)
  equalize_cdf_apply_kernel, table fallback test_float_equalize_group_counts[65536], test_float_equalize_flat_frames
                                            (level 12345)
  lab_histogram_fast_kernel                 test_lab_stretch_one_call[1024x1024], [17x61681] (label colorspace_histogram)
"""
import numpy as np
import pytest

from conftest import make_pixels, to_device, assert_parity
from oracle import restate as R

pytestmark = pytest.mark.gpu

Q16, HDRI = np.uint16, np.float32
SMALL = (37, 41)
# the launchers switch kernels at 1 << 20 pixels (histogram_typed, launch_apply_lut, apply_histogram_lut and the fused
# Lab launchers): one pixel below, on it, one above
THRESHOLD = 1 << 20
LARGE_SHAPES = [(1023, 1025), (1024, 1024), (17, 61681)]
DEGENERATE_SHAPES = [(1, 1), (1, 2), (3, 1), (5, 7), (1, 1025), (257, 1)]
# histogram_packed_kernel: 16-bit counters two to a word, kPackedCapacity pixels a workgroup; packed_histogram_blocks
# starts more workgroups than compute units once a share passes the capacity + 256
PACKED_CAPACITY = 65534
COMPUTE_UNITS = 256
BIG_PACKED_SHAPE = (4105, 4105)
CARRY_LEVELS = (30001, 30000)                 # odd, then the even level below it: one LDS word
HIST_HALF = 32768                             # histogram_lds_kernel's two passes
# equalize_cdf_apply_kernel: uint16 offsets inside groups of 16 bins, `d > 65535u` sends the workgroup to the table
GROUP = 16
GROUP_FIRST_BIN = 12800
GROUP_COUNTS = (65535, 65536)
FLAT_LEVELS = (12352, 12345)                  # first bin of its group (running counts), ninth (table)

Q16_PLANTED = [0, 1, 32767, 32768, 65534, 65535]
FLOAT_PLANTED = [-3.0, -0.0, 1e-40, 0.49, 0.5, 1.5, 2.5, 12344.5, 65534.49, 65534.5, 65535.0, 65535.5, 70000.0]
FLOAT_PLANTED_PER_CHANNEL = FLOAT_PLANTED + [np.inf, -np.inf]

CHANNEL_BITS = {"R": 0x1, "G": 0x2, "B": 0x4, "A": 0x10}
STRETCH_MASKS = ["R", "G", "A", "RGB", "RGBA"]
EQUALIZE_MASKS = [None, "RGB", "RGB,sync", "A"]


def level_pairs(n):
    """(black_point, white_point) of part A."""
    return [(0.0, float(n)), (0.0, 0.0), (float(n), float(n)), (n + 5.0, float(n)), (n - 1.0, float(n)),
            (0.7 * n, 0.3 * n), (-1.0, n + 1.0)]


def mask_arguments(im, mask, channels):
    """The product's (channel_mask, copy_channels) for the reference's -channel string (None: the default mask)."""
    if mask is None:
        return im.ALL_CHANNELS, ()
    letters, _, flag = mask.partition(",")
    value = sum(CHANNEL_BITS[letter] for letter in letters) | (im.SYNC_CHANNELS if flag == "sync" else 0)
    index = {"R": 0, "G": 1, "B": 2, "A": channels - 1 if channels in (2, 4) else None}
    updated = {index[letter] for letter in letters} - {None}
    return value, tuple(c for c in range(channels) if c not in updated)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(got, want, what):
    assert_parity(got, want, True, what)
    if want.dtype == np.float32:
        differ = got.view(np.uint32) != want.view(np.uint32)
        assert not differ.any(), "%s: %d bit patterns differ, first at %s" % (what, int(differ.sum()), np.argwhere(differ)[0].tolist())


def stretch(black, white):
    return ("stretch", black, white)


EQUALIZE = ("equalize",)


def reference(refmod, px, op, mask=None, colorspace="sRGB"):
    ref = refmod.RefImage(px, colorspace)
    if mask is not None:
        ref.set_channel_mask(mask)
    return (ref.equalize() if op[0] == "equalize" else ref.contrast_stretch(op[1], op[2])).numpy()


def on_device(im, px, op, mask=None, colorspace="sRGB", precision=None, host=False):
    channel_mask, copy = mask_arguments(im, mask, px.shape[2])
    image = im.Image(px.copy() if host else to_device(px), colorspace=colorspace, channel_mask=channel_mask,
                     copy_channels=copy, precision=precision)
    if op[0] == "equalize":
        im.equalize_image(image)
    else:
        im.contrast_stretch_image(image, op[1], op[2])
    return image.numpy()


def check(im, refmod, px, op, mask=None, what="", want=None, colorspace="sRGB"):
    """Both precisions against the reference's result (computed once); returns it."""
    if want is None:
        want = reference(refmod, px, op, mask, colorspace)
    for precision in (im.PRECISION_EXACT, im.PRECISION_FAST):
        got = on_device(im, px, op, mask, colorspace, precision)
        same_bits(got, want, "%s %s mask %s precision %d" % (what, op, mask, precision))
    return want


def colour(px):
    """A pixel with R != G (frames of three or more channels)."""
    if px.shape[2] >= 3:
        px[0, 0, 0], px[0, 0, 1] = 1000, 2000
    return px


def frame(shape, channels, dtype, kind="random", seed=42):
    return colour(make_pixels(shape[0], shape[1], channels, dtype, seed=seed, kind=kind))


# ----------------------------------------------------------------------------------- A. level-scan edges
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_level_scan_edges(im, refmod, options, dtype, channels, kind):
    """The scans of enhance.c:1663-1677 at their ends: a white scan that stops at 0, a black scan that runs off the
    table (j = 65536: 0 as a Q16 Quantum, 65536 as a float one, so every float sample maps to 0), black > white, and
    negative thresholds, per sample (stretch_apply_levels_kernel) and tabulated (lut_stretch_map_kernel)."""
    px = frame(SMALL, channels, dtype, kind, seed=7 + channels)
    n = SMALL[0] * SMALL[1]
    wants = [check(im, refmod, px, stretch(b, w), what="levels") for b, w in level_pairs(n)]
    if dtype == HDRI:
        assert not wants[2].any() and not wants[3].any()       # black = 65536: j < black everywhere
    options.set("MAGICKHIP_NO_STRETCH_LEVELS")
    for (b, w), want in zip(level_pairs(n), wants):
        check(im, refmod, px, stretch(b, w), what="tabulated", want=want)


def tie_frame(channels, dtype):
    """Exactly 100 pixels at the lowest level (0) and 100 at the highest (65535); the rest strictly between."""
    rows, cols = SMALL
    rng = np.random.default_rng(23)
    px = rng.integers(1000, 60000, (rows, cols, channels)).astype(dtype)
    flat = px.reshape(-1, channels)
    where = rng.permutation(rows * cols)
    flat[where[:100]] = 0
    flat[where[100:200]] = 65535
    if channels >= 3:
        flat[where[200]][:2] = (1000, 2000)
    return px


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 4])
def test_tie_frame(im, refmod, options, dtype, channels):
    """The strict `>` of both scans: a threshold that EQUALS the running count of the end bin moves the level to the
    next occupied bin, a threshold just below it does not."""
    px = tie_frame(channels, dtype)
    n = SMALL[0] * SMALL[1]
    idx = R.scale_quantum_to_map(R.clamp_to_quantum(R.pixel_intensity(px), dtype == HDRI), dtype == HDRI)
    counts = np.bincount(idx.ravel(), minlength=65536)
    assert counts[0] == 100 and counts[65535] == 100
    cases = [(100.0, float(n)), (99.999, float(n)), (100.001, float(n)),
             (0.0, n - 100.0), (0.0, n - 99.999), (0.0, n - 100.001)]
    wants = [check(im, refmod, px, stretch(b, w), what="tie") for b, w in cases]
    # the thresholds land on different bins: the reference's own results differ (black), (white)
    assert not np.array_equal(wants[0], wants[1]) and np.array_equal(wants[0], wants[2])
    assert not np.array_equal(wants[3], wants[4]) and np.array_equal(wants[3], wants[5])
    options.set("MAGICKHIP_NO_STRETCH_LEVELS")
    for (b, w), want in zip(cases, wants):
        check(im, refmod, px, stretch(b, w), what="tie, tabulated", want=want)


def one_bin_frame(channels, dtype, ramp):
    """All but three pixels at one colour with R != G; ramp: the green channel holds distinct levels instead."""
    rows, cols = SMALL
    px = np.empty((rows, cols, channels), dtype=dtype)
    px[:, :] = (30000, 20000, 10000, 40000)[:channels]
    px[0, 0, :3] = (100, 200, 300)                  # one pixel below
    px[5, 5, :3] = (60000, 61000, 62000)            # two above
    px[rows - 1, cols - 1, :3] = (50000, 51000, 52000)
    if ramp:
        px[:, :, 1] = (np.arange(rows * cols).reshape(rows, cols) * 13 % 50000 + 500).astype(dtype)
    return px


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [3, 4])
def test_one_bin_frame(im, refmod, options, dtype, channels):
    """All but three pixels at one colour: black == white on the shared histogram and the frame comes back untouched
    (enhance.c:1782); under a per-channel mask only the channels that collapse are left alone."""
    n = SMALL[0] * SMALL[1]
    px = one_bin_frame(channels, dtype, False)
    want = check(im, refmod, px, stretch(2.0, n - 2.0), what="one bin")
    assert np.array_equal(want, px)
    # per channel: R and B collapse, G holds a ramp and is stretched
    px = one_bin_frame(channels, dtype, True)
    masked = check(im, refmod, px, stretch(2.0, n - 2.0), "RGB", what="one bin per channel")
    assert np.array_equal(masked[:, :, 0], px[:, :, 0]) and np.array_equal(masked[:, :, 2], px[:, :, 2])
    assert not np.array_equal(masked[:, :, 1], px[:, :, 1])
    options.set("MAGICKHIP_NO_STRETCH_LEVELS")
    check(im, refmod, px, stretch(2.0, n - 2.0), "RGB", what="one bin per channel, tabulated", want=masked)
    px = one_bin_frame(channels, dtype, False)
    check(im, refmod, px, stretch(2.0, n - 2.0), what="one bin, tabulated", want=px)


# ----------------------------------------------------------------------------------- B. binning edges
def planted_frame(channels, dtype, per_channel):
    px = frame(SMALL, channels, dtype, "random", seed=11)
    values = Q16_PLANTED if dtype == Q16 else (FLOAT_PLANTED_PER_CHANNEL if per_channel else FLOAT_PLANTED)
    flat = px.reshape(-1)
    flat[:len(values)] = np.array(values, dtype=dtype)
    flat[-len(values):] = np.array(values[::-1], dtype=dtype)
    if channels >= 3:
        px[2, 2, :2] = (1000, 2000)
    return px


def restated_bins(px, per_channel):
    """oracle.restate's own binning: [65536, channels] counts."""
    hdri = px.dtype == np.float32
    out = np.zeros((65536, px.shape[2]), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(px.shape[2]):
            v = px[:, :, c].astype(np.float64) if per_channel else R.pixel_intensity(px)
            idx = R.scale_quantum_to_map(R.clamp_to_quantum(v, hdri), hdri)
            out[:, c] = np.bincount(np.asarray(idx).ravel(), minlength=65536)
    return out


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("per_channel", [False, True])
def test_binning_edges(im, refmod, dtype, channels, per_channel):
    """ScaleQuantumToMap's clamps and its +0.5f rounding (quantum-private.h:504-514) on samples at and beside every
    edge, in the first and in the last pixels of the frame, binned by intensity and per channel, for both operators;
    the table itself against a bincount of the restatement's bins."""
    px = planted_frame(channels, dtype, per_channel)
    n = SMALL[0] * SMALL[1]
    mask = {1: "R", 3: "RGB", 4: "RGBA"}[channels] if per_channel else None
    table = im.histogram(im.Image(to_device(px)), not per_channel).cpu().numpy()
    assert np.array_equal(table, restated_bins(px, per_channel))
    assert (table.sum(axis=0) == n).all()
    for b, w in ((0.02 * n, n - 0.01 * n), (0.0, float(n)), (float(n), float(n))):
        check(im, refmod, px, stretch(b, w), mask, what="planted")
    check(im, refmod, px, EQUALIZE, mask, what="planted")


# ----------------------------------------------------------------------------------- C. channel masks
def run_masks(im, refmod, px, what):
    n = px.shape[0] * px.shape[1]
    for mask in STRETCH_MASKS:
        want = check(im, refmod, px, stretch(0.03 * n, n - 0.02 * n), mask, what=what)
        _, copy = mask_arguments(im, mask, px.shape[2])
        for c in copy:
            assert np.array_equal(bits(want[:, :, c]), bits(px[:, :, c])), (mask, c)
    for mask in EQUALIZE_MASKS:
        want = check(im, refmod, px, EQUALIZE, mask, what=what)
        _, copy = mask_arguments(im, mask, px.shape[2])
        for c in copy:
            assert np.array_equal(bits(want[:, :, c]), bits(px[:, :, c])), (mask, c)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_masks_on_small_frames(im, refmod, dtype, channels, kind):
    """Per-channel tables (a mask other than AllChannels: enhance.c:1640-1641; no SyncChannels: :2125-2127), `RGBA`
    (not AllChannels: alpha is stretched from its own table), `RGB,sync` (the intensity table, alpha copied) and
    single channels; what the mask leaves out comes back bit for bit."""
    run_masks(im, refmod, frame(SMALL, channels, dtype, kind, seed=3), "small")


def large_frame(channels, dtype, kind):
    rows = cols = 1024
    if kind == "smooth":
        return frame((rows, cols), channels, dtype, "smooth", seed=5)
    rng = np.random.default_rng(31)
    if kind == "runs32":
        levels = rng.integers(0, 65536, (rows, cols // 32, channels))
        px = np.repeat(levels, 32, axis=1)
    else:                                            # period2: neighbouring pixels never agree
        a = rng.integers(0, 32768, (rows, 1, channels))
        b = rng.integers(32768, 65536, (rows, 1, channels))
        px = np.where((np.arange(cols) % 2 == 0)[None, :, None], a, b)
    return colour(np.ascontiguousarray(px.astype(dtype)))


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("kind", ["smooth", "runs32", "period2"])
def test_masks_on_large_frames(im, refmod, dtype, channels, kind):
    """The same masks at 2^20 pixels, where per-channel binning stays on histogram_kernel with global atomics: runs
    of 32 equal pixels send histogram_add through its leader election (>= 16 agreeing lanes), levels alternating
    with period 2 do not."""
    run_masks(im, refmod, large_frame(channels, dtype, kind), kind)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [3, 4])
def test_flat_frame_of_65_pixels(im, refmod, dtype, channels):
    """One colour, 65 pixels: the second wave holds one valid lane beside 63 invalid ones that load the same pixel."""
    px = np.empty((5, 13, channels), dtype=dtype)
    px[:, :] = (30000, 20000, 10000, 40000)[:channels]
    for mask in [None] + STRETCH_MASKS:
        for b, w in ((0.0, 65.0), (65.0, 65.0)):
            check(im, refmod, px, stretch(b, w), mask, what="flat 65")
    for mask in EQUALIZE_MASKS:
        check(im, refmod, px, EQUALIZE, mask, what="flat 65")


# ----------------------------------------------------------------------------------- D. size thresholds
def both_operators(im, refmod, px, what, options=None, also_unpacked=False):
    n = px.shape[0] * px.shape[1]
    ops = [stretch(0.02 * n, n - 0.01 * n), stretch(float(n), float(n)), EQUALIZE]
    wants = [check(im, refmod, px, op, what=what) for op in ops]
    if also_unpacked:
        options.set("MAGICKHIP_NO_PACKED_HISTOGRAM")
        for op, want in zip(ops, wants):
            check(im, refmod, px, op, what=what + ", half-range histogram", want=want)
    return ops, wants


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_size_thresholds(im, refmod, options, shape, channels, dtype):
    """2^20 - 1, 2^20 and 2^20 + 1 pixels: the histogram kernel, the apply kernel and the float-equalize kernel
    change together at 1 << 20; the packed and the half-range histogram agree with the reference, hence with each
    other; the tabulated stretch takes apply_lut_shared_kernel on the Q16 frames of 2^20 pixels and more."""
    px = frame(shape, channels, dtype, "random", seed=shape[1])
    ops, wants = both_operators(im, refmod, px, "%dx%d" % shape, options, also_unpacked=True)
    options.set("MAGICKHIP_NO_STRETCH_LEVELS")
    for op, want in zip(ops[:2], wants[:2]):
        check(im, refmod, px, op, what="%dx%d tabulated" % shape, want=want)


@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
def test_degenerate_shapes(im, refmod, shape, dtype):
    for channels in (1, 2, 3, 4):
        both_operators(im, refmod, frame(shape, channels, dtype, "random", seed=shape[0] + channels), "%dx%d" % shape)


def test_packed_counter_carry(im, refmod, options):
    """A workgroup's whole share in the HIGH half of one LDS word (an odd level), the later workgroups' in its LOW
    half (the even level below): a carry out of the low counter would show in the high one."""
    px = np.empty((1024, 1024, 1), dtype=Q16)
    px[:512], px[512:] = CARRY_LEVELS
    table = im.histogram(im.Image(to_device(px)), True).cpu().numpy()
    assert table[CARRY_LEVELS[0], 0] == table[CARRY_LEVELS[1], 0] == THRESHOLD // 2 and table.sum() == THRESHOLD
    both_operators(im, refmod, px, "carry", options, also_unpacked=True)


def test_packed_more_workgroups_than_compute_units(im, refmod):
    """4105 x 4105: a share of one workgroup per compute unit passes the 16-bit counters' capacity, so
    packed_histogram_blocks starts ceil(n / kPackedCapacity) workgroups."""
    px = make_pixels(BIG_PACKED_SHAPE[0], BIG_PACKED_SHAPE[1], 1, Q16, seed=77)
    table = im.histogram(im.Image(to_device(px)), True).cpu().numpy()
    assert np.array_equal(table[:, 0], np.bincount(px.ravel(), minlength=65536))
    n = px.shape[0] * px.shape[1]
    for op in (stretch(0.02 * n, n - 0.01 * n), EQUALIZE):
        same_bits(on_device(im, px, op), reference(refmod, px, op), "4105x4105 %s" % (op,))


# ----------------------------------------------------------------------------------- E. float equalize from running counts
def group_frame(channels, count):
    """1024 x 1040 float: `count` pixels in bins GROUP_FIRST_BIN+1 .. +15, none else in them."""
    rows, cols = 1024, 1040
    rng = np.random.default_rng(count)
    g = rng.integers(0, 65536, rows * cols).astype(np.float32)
    inside = (g > GROUP_FIRST_BIN) & (g < GROUP_FIRST_BIN + GROUP)
    g[inside] = GROUP_FIRST_BIN
    g[:count] = GROUP_FIRST_BIN + 1 + np.arange(count) % (GROUP - 1)
    px = np.repeat(g.reshape(rows, cols, 1), channels, axis=2)
    if channels == 4:
        px[:, :, 3] = rng.integers(0, 65536, (rows, cols)).astype(np.float32)
    return np.ascontiguousarray(px)


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("count", GROUP_COUNTS)
def test_float_equalize_group_counts(im, refmod, options, channels, count):
    """Either side of `d > 65535u`: 65 535 pixels above the first bin of one 16-bin group fit the uint16 offsets,
    65 536 send the workgroups to the table.  Both must be the reference's bits, with and without the running-counts
    kernel."""
    px = group_frame(channels, count)
    bins = restated_bins(px, False)[:, 0]
    assert bins[GROUP_FIRST_BIN + 1:GROUP_FIRST_BIN + GROUP].sum() == count
    want = check(im, refmod, px, EQUALIZE, what="group of %d" % count)
    options.set("MAGICKHIP_NO_EQUALIZE_COUNTS")
    check(im, refmod, px, EQUALIZE, what="group of %d, table" % count, want=want)


@pytest.mark.parametrize("level", FLAT_LEVELS)
def test_float_equalize_flat_frames(im, refmod, options, level):
    """A flat non-zero frame maps every sample to 65535; an all-zero frame has black == white and comes back
    untouched (enhance.c:2164, :2254)."""
    flat = np.full((1024, 1024, 1), level, dtype=HDRI)
    zero = np.zeros((1024, 1024, 1), dtype=HDRI)
    rgba = np.empty((1024, 1024, 4), dtype=HDRI)
    rgba[:, :] = (level, level + 100.0, level - 50.0, 777.0)
    for name, px in (("flat", flat), ("zero", zero), ("flat rgba", rgba)):
        want = check(im, refmod, px, EQUALIZE, what=name)
        if name == "zero":
            assert np.array_equal(want, px)
        elif name == "flat":
            assert (want == 65535.0).all()
    options.set("MAGICKHIP_NO_EQUALIZE_COUNTS")
    for name, px in (("flat", flat), ("zero", zero)):
        check(im, refmod, px, EQUALIZE, what=name + ", table")


def test_equalize_flat_frames_q16(im, refmod):
    for level in (FLAT_LEVELS[1], 0):
        px = np.full((SMALL[0], SMALL[1], 1), level, dtype=Q16)
        want = check(im, refmod, px, EQUALIZE, what="flat %d" % level)
        assert (want == (65535 if level else 0)).all()


# ----------------------------------------------------------------------------------- F. one table over two row bands
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_one_table_over_two_row_bands(im, refmod, dtype):
    """The sharded path's contract on one device: both bands accumulate into one table, each band is mapped from it
    with the whole frame's row count (white_point counts pixels of the frame, not of the band)."""
    rows, cols, split = 173, 96, 80
    px = frame((rows, cols), 4, dtype, "smooth", seed=9)
    n = rows * cols
    for op in (EQUALIZE, stretch(0.02 * n, n - 0.01 * n), stretch(0.7 * n, 0.3 * n)):
        bands = [im.Image(to_device(np.ascontiguousarray(px[:split]))), im.Image(to_device(np.ascontiguousarray(px[split:])))]
        table = im.histogram(bands[0], True)
        im.histogram(bands[1], True, out=table)
        assert int(table[:, 0].sum()) == n
        for band in bands:
            if op[0] == "equalize":
                im.apply_histogram(band, table, True, True, image_rows=rows)
            else:
                im.apply_histogram(band, table, True, False, op[1], op[2], image_rows=rows)
        got = np.concatenate([band.numpy() for band in bands], axis=0)
        same_bits(got, reference(refmod, px, op), "two bands %s" % (op,))


# ----------------------------------------------------------------------------------- G. the gray decline
@pytest.mark.parametrize("dtype", [Q16, HDRI])
@pytest.mark.parametrize("channels,host", [(3, False), (4, False), (4, True)])
def test_gray_frames_are_declined(im, refmod, dtype, channels, host):
    """IdentifyImageType's side effect (enhance.c:1586-1588) is the caller's: an all-gray sRGB frame is handed back
    untouched with an error; the same pixels marked Lab are not scanned and are stretched."""
    rows, cols = SMALL
    n = rows * cols
    gray = make_pixels(rows, cols, 1, dtype, seed=13, kind="smooth")
    px = np.ascontiguousarray(np.repeat(gray, channels, axis=2))
    if channels == 4:
        px[:, :, 3] = make_pixels(rows, cols, 1, dtype, seed=14)[:, :, 0]
    image = im.Image(px.copy() if host else to_device(px))
    with pytest.raises(im.MagickHipError):
        im.contrast_stretch_image(image, 0.02 * n, n - 0.01 * n)
    assert np.array_equal(bits(image.numpy()), bits(px))
    op = stretch(0.02 * n, n - 0.01 * n)
    want = reference(refmod, px, op, colorspace="Lab")
    assert not np.array_equal(want, px)
    same_bits(on_device(im, px, op, colorspace="Lab", host=host), want, "gray pixels marked Lab")


# ----------------------------------------------------------------------------------- H. host memory
@pytest.mark.parametrize("dtype", [Q16, HDRI])
def test_host_memory(im, refmod, dtype):
    px = frame(SMALL, 4, dtype, "smooth", seed=21)
    n = SMALL[0] * SMALL[1]
    for op, mask in ((stretch(0.7 * n, 0.3 * n), None), (stretch(float(n), float(n)), None), (EQUALIZE, None),
                     (stretch(0.03 * n, n - 0.02 * n), "RGB"), (EQUALIZE, "RGB")):
        same_bits(on_device(im, px, op, mask, host=True), reference(refmod, px, op, mask), "host %s %s" % (op, mask))


# ----------------------------------------------------------------------------------- I. the one-call Lab + stretch
@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_lab_stretch_one_call(im, refmod, shape):
    """FAST sRGB -> Lab + ContrastStretch on RGBA Q16 in one call: the Lab frame is FAST's (within one level of the
    reference), the stretch is the reference's own on THAT frame, bit for bit; at 2^20 pixels and above the call
    converts and bins in one kernel (lab_histogram_fast_kernel), below it runs the two operators."""
    import bench
    px = frame(shape, 4, Q16, "random", seed=shape[0])
    n = shape[0] * shape[1]
    lab = im.Image(to_device(px), precision=im.PRECISION_FAST)
    im.transform_image_colorspace(lab, "Lab")
    device_lab = lab.numpy().copy()
    assert_parity(device_lab, refmod.RefImage(px).colorspace("Lab").numpy(), False, "FAST Lab")
    for b, w in ((0.0, float(n)), (0.7 * n, 0.3 * n), (float(n), float(n))):
        image = im.Image(to_device(px), precision=im.PRECISION_FAST)
        launched = set(bench.kernel_profile(im, lambda: im.transform_colorspace_contrast_stretch_image(image, "Lab", b, w), 1))
        assert ("colorspace_histogram" in launched) == (n >= THRESHOLD), launched
        want = refmod.RefImage(device_lab, "Lab").contrast_stretch(b, w).numpy()
        same_bits(image.numpy(), want, "Lab + stretch %g %g" % (b, w))
