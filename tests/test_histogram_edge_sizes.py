"""Keeps the sizes of tests/test_gpu_histogram_edges.py tied to the constants of the kernels they are meant to straddle,
without a GPU: the `1 << 20` switches of the launchers, kPackedCapacity, kHistHalf and the 16-bin group of
equalize_cdf_apply_kernel, read from histogram.hip and operators_enhance.cpp the way tests/test_enhance_edge_sizes.py
reads its constants.  Whoever moves one of them gets a failure here instead of a GPU test that quietly stops covering
both sides."""
import re

import test_gpu_histogram_edges as edges
from test_enhance_edge_sizes import source, function_body

SWITCH = "((size_t) 1 << 20)"


def test_large_shapes_straddle_the_megapixel_switches():
    text = source("histogram.hip")
    assert "(mode != 0) && (n >= %s)" % SWITCH in function_body(text, "static MhStatus histogram_typed(")
    assert "(img.columns*img.rows >= %s)" % SWITCH in function_body(text, "MhStatus launch_apply_lut(")
    # the two fused Lab launchers share one gate
    assert "(n < %s)" % SWITCH in function_body(text, "static size_t lab_histogram_fast_blocks(")
    for launcher in ("MhStatus launch_lab_fast_with_histogram(", "MhStatus launch_lab_fast_contrast_stretch("):
        assert "lab_histogram_fast_blocks(img)" in function_body(text, launcher)
    enhance = function_body(source("operators_enhance.cpp"), "MhStatus apply_histogram_lut(")
    assert "(view.columns*view.rows >= %s)" % SWITCH in enhance
    assert edges.THRESHOLD == 1 << 20
    assert [rows * cols - edges.THRESHOLD for rows, cols in edges.LARGE_SHAPES] == [-1, 0, 1]
    assert all(rows * cols < edges.THRESHOLD for rows, cols in edges.DEGENERATE_SHAPES + [edges.SMALL])
    # the batched kernels load four pixels a thread with clamped indices: a ragged last batch on either side
    assert any((rows * cols) % 4 != 0 for rows, cols in edges.LARGE_SHAPES)
    for kernel in ("stretch_apply_levels_kernel(Q *pixels", "apply_lut_shared_kernel(uint16_t *pixels",
                   "equalize_cdf_apply_kernel(float *pixels"):
        assert "(i < npixels ? i : npixels-1)" in function_body(text, "void " + kernel)


def test_packed_counter_cases_follow_the_capacity():
    text = source("histogram.hip")
    capacity = int(re.search(r"constexpr unsigned kPackedCapacity=(\d+)u;", text).group(1))
    assert capacity == edges.PACKED_CAPACITY and capacity < 65536 and capacity % 2 == 0
    blocks = function_body(text, "static size_t packed_histogram_blocks(int device,size_t n)")
    assert "if ((n+nblocks-1)/nblocks > kPackedCapacity+256u)" in blocks
    assert "nblocks=(n+kPackedCapacity-1)/kPackedCapacity;" in blocks and "nblocks > 65536 ? 0 : nblocks" in blocks
    cus = edges.COMPUTE_UNITS
    # the three threshold frames and the carry frame: one workgroup per compute unit, its share inside the counters
    for rows, cols in edges.LARGE_SHAPES:
        assert (rows * cols + cus - 1) // cus <= capacity
    # the big frame: a share per compute unit past capacity + 256, so more workgroups than compute units
    n = edges.BIG_PACKED_SHAPE[0] * edges.BIG_PACKED_SHAPE[1]
    assert (n + cus - 1) // cus > capacity + 256
    assert cus < (n + capacity - 1) // capacity <= 65536
    # the carry case: both levels in one LDS word, the odd one in its high half (bin >> 1, bin & 1)
    kernel = function_body(text, "void histogram_packed_kernel(")
    assert "atomicAdd(table+(bin >> 1),(bin & 1u) != 0u ? 0x10000u : 1u);" in kernel
    odd, even = edges.CARRY_LEVELS
    assert odd % 2 == 1 and even == odd - 1 and odd >> 1 == even >> 1


def test_planted_samples_sit_on_both_sides_of_the_half_range():
    text = source("histogram.hip")
    half = int(re.search(r"constexpr int kHistHalf=(\d+);", text).group(1))
    assert half == edges.HIST_HALF == 32768
    assert "const unsigned base=(unsigned) half*kHistHalf;" in function_body(text, "void histogram_lds_kernel(")
    assert {half - 1, half, 0, 65535} <= set(edges.Q16_PLANTED)


def test_group_counts_straddle_the_equalize_fallback():
    kernel = function_body(source("histogram.hip"), "void equalize_cdf_apply_kernel(")
    assert "first=cdf[j & ~15];" in kernel and "base[j >> 4]" in kernel and "if (d > 65535u)" in kernel
    assert edges.GROUP == 16 and edges.GROUP_FIRST_BIN % edges.GROUP == 0
    assert edges.GROUP_COUNTS == (65535, 65536)
    counts, table = edges.FLAT_LEVELS
    assert counts % edges.GROUP == 0 and table % edges.GROUP != 0
    assert 1024 * 1024 > 65535                      # the flat frames: a whole frame in one bin
