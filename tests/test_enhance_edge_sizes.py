"""Keeps the big-frame and block-boundary cases of tests/test_gpu_enhance_edges.py honest without a GPU: their sizes
follow constants of the kernels' sources (stream_grid's block cap, the 256-thread block, kPointBatch), read here from
layout_dispatch.hpp, pointwise.hip and effects.hip the way the *_kernel_resources modules read ISA facts.  Whoever changes one of them
gets a failure here instead of a GPU test that quietly stops covering the second trip of a grid-stride loop.  Also
draws the first cases of the stress families 16 to 18 (no GPU needed: the decline conditions depend on shape and
radius only) and checks the share of declined cases against the quarter the driver allows."""
import os
import re

import numpy as np

import test_gpu_enhance_edges as edges

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "imagemagick_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(text, signature):
    """The text from `signature` to the closing brace of the function it opens."""
    start = text.index(signature)
    brace = text.index("{", start)
    depth, i = 0, brace
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[start:i + 1]
        i += 1


def kernel_launch_bounds(text, kernel):
    """The __launch_bounds__ in front of `void kernel(`."""
    m = re.search(r"__launch_bounds__\((\d+)\)\s*void\s+%s\s*\(" % re.escape(kernel), text)
    assert m, "no __launch_bounds__ in front of %s" % kernel
    return int(m.group(1))


def pointwise_constants():
    geometry = source("layout_dispatch.hpp")
    grid = function_body(geometry, "static unsigned stream_grid(size_t npixels)")
    block = re.search(r"blocks=\(npixels\+(\d+)\)/(\d+);", grid)
    cap = re.search(r"if \(blocks > (\d+)\)\s*blocks=(\d+);", grid)
    batch = re.search(r"constexpr int kPointBatch=(\d+);", geometry)
    assert block and cap and batch
    assert int(block.group(1)) + 1 == int(block.group(2)) and cap.group(1) == cap.group(2)
    return int(cap.group(1)), int(block.group(2)), int(batch.group(1)), source("pointwise.hip")


def test_big_frames_sit_just_above_one_trip_of_the_grid_stride_loops():
    cap, width, batch, text = pointwise_constants()
    assert (cap, width, batch) == (edges.STREAM_CAP_BLOCKS, edges.BLOCK_WIDTH, edges.POINT_BATCH)
    # the three kernels run `width` threads a block on stream_grid's grid; tone_kernel on a grid for n/kPointBatch
    for kernel in ("function_kernel", "grayscale_kernel", "tone_kernel"):
        assert kernel_launch_bounds(text, kernel) == width
    for launch, label in (("MhStatus launch_function(", "function_kernel"), ("MhStatus launch_grayscale(", "grayscale_kernel")):
        body = function_body(text, launch)
        assert "dim3(stream_grid(n)),dim3(%d)" % width in body and label in body
    tone = function_body(text, "static MhStatus launch_tone(")
    assert "dim3 grid(stream_grid((n+kPointBatch-1)/kPointBatch)),block(%d);" % width in tone
    kernel = function_body(text, "void tone_kernel(Q *__restrict__ pixels,size_t npixels,ToneArgs a)")
    assert "(ik < npixels ? ik : npixels-1)" in kernel and "if (i < npixels)" in kernel
    one = cap * width
    n = edges.BIG_STREAM_SHAPE[0] * edges.BIG_STREAM_SHAPE[1]
    assert one < n < 1.02 * one
    n = edges.BIG_TONE_SHAPE[0] * edges.BIG_TONE_SHAPE[1]
    assert one * batch < n < 1.02 * one * batch
    assert n % (width * batch) != 0                       # a ragged last batch: clamped loads, guarded stores
    assert edges.GUARD_ROWS * edges.BIG_TONE_SHAPE[1] >= width * batch        # what a batch could overrun stays inside the guard


def column_constants():
    """kColumnBlock and the one-thread-per-column grid of layout_dispatch.hpp."""
    geometry = source("layout_dispatch.hpp")
    block = re.search(r"constexpr int kColumnBlock=(\d+);", geometry)
    assert block
    grid = function_body(geometry, "static inline dim3 column_grid(size_t columns,size_t rows=1)")
    assert "return dim3((unsigned) ((columns+kColumnBlock-1)/kColumnBlock),(unsigned) rows);" in grid
    return int(block.group(1))


def test_block_boundary_widths_follow_the_kernels_block_width():
    text = source("effects.hip")
    kernels = ["motion_blur_kernel", "rotational_blur_kernel", "local_contrast_luma_kernel", "local_contrast_vertical_kernel",
               "local_contrast_horizontal_kernel", "despeckle_load_kernel", "hull_kernel", "despeckle_store_kernel",
               "wavelet_hat_kernel"]
    widths = {kernel_launch_bounds(text, k) for k in kernels}
    assert widths == {edges.BLOCK_WIDTH}
    b = edges.BLOCK_WIDTH
    assert column_constants() == b                        # the launchers' block is the kernels' launch bound
    # the launches: one thread per column (despeckle_load: per padded column, wavelet_hat: per column and colour channel)
    motion = function_body(text, "MhStatus launch_motion_blur(")
    assert "column_grid(a.columns,a.rows)" in motion and "dim3(kColumnBlock)" in motion and "motion_blur_kernel<" in motion
    rotational = function_body(text, "MhStatus launch_rotational_blur(")
    assert "column_grid(a.columns,a.rows)" in rotational and "dim3(kColumnBlock)" in rotational
    assert "rotational_blur_kernel<" in rotational
    local = function_body(text, "MhStatus launch_local_contrast(")
    assert "const dim3 block(kColumnBlock),grid=column_grid(a.columns,a.rows);" in local
    assert "column_grid(a.columns,a.rows+2*a.w),block" in local
    despeckle = function_body(text, "static MhStatus despeckle_typed(")
    assert "const dim3 block(kColumnBlock);" in despeckle and "column_grid(W+2,H+2),block" in despeckle
    assert "const dim3 grid=column_grid(W,H);" in despeckle
    wavelet = function_body(text, "MhStatus launch_wavelet_denoise(")
    assert "const dim3 block(kColumnBlock);" in wavelet and "const dim3 grid=column_grid(W*colour,H);" in wavelet
    # no launch of these files' kernels with a block or grid spelled by hand
    assert not re.search(r"block\(\d+\)|dim3\(\d+\)|\+\d+\)/\d+", text)
    w = edges.BOUNDARY_WIDTHS
    assert {b - 1, b, b + 1} <= set(w)                    # one below, on and one above a block
    assert 2 * b + 1 in w and any(b + 1 < v < 2 * b for v in w)      # a third block of one column; a ragged second block
    assert {b - 2, b - 1} <= set(w)                       # despeckle_load_kernel: W+2 on and one above a block
    assert any(v < b < 3 * v for v in w) and b + 1 in w   # wavelet_hat_kernel: W*colour crosses a block with colour 3 and 1
    # the decline thresholds the GPU tests restate
    assert "if ((W < 33) || (H < 33))" in wavelet
    assert "if ((a.w < 1) || (a.columns <= 2*a.w+2))" in local
    assert "a.w=(int) (long) ((double) longest*0.002*fabs(radius));" in local


def test_stress_families_decline_at_most_a_quarter_of_their_cases():
    """The first 300 cases of the seeds the suite's slice uses (6000 + family)."""
    import stress_parity
    shares = {}
    for op in (16, 17, 18):
        stress_parity.rng = np.random.default_rng(6000 + op)
        stress_parity.declined.pop(op, None)
        stress_parity.drawn.pop(op, None)
        for case in range(300):
            stress_parity.draw_frame()
            drawn = stress_parity.draw_enhance_case(op)
            assert drawn["frame"].dtype in (np.uint16, np.float32)
            # never above the cap at any point of the run (the driver allows three before the twelfth case)
            assert 4 * stress_parity.declined.get(op, 0) <= max(case + 1, 12)
        shares[op] = stress_parity.declined.get(op, 0) / 300.0
        stress_parity.declined.pop(op, None)
        stress_parity.drawn.pop(op, None)
    print("declined share of families 16, 17, 18:", shares)
    assert shares[16] == 0.0 and shares[17] == 0.0       # nothing in them is declined
    assert 0.0 < shares[18] <= 0.25                       # LocalContrastImage's two thresholds are reached, within the cap
