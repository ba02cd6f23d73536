"""The FAST one-launch resize kernels keep their device-side plans in most-recently-used caches of 16 entries
(resize_stream.hip, resize_mfma.hip; mru_cache.hpp), which no other test fills: more geometries than a cache holds,
one after the other and from four threads at once, each result against RefImage.resize under FAST's contract (within
one Quantum level or one float ULP).  An evicted plan is destroyed while its kernels may still be queued on another
stream, and rebuilt when its geometry comes back.  The walk: a 37x23 RGBA frame to 74 columns (x2 across: the
streaming form) and to 85 columns (x2.3: the matrix form), 18 row counts each whose factor is not below the horizontal
one, so that the vertical filter runs first; tests/cpu/resize_stream_plan_test.cpp and resize_mfma_plan_test.cpp
build the plans of both ends of each walk on the host."""
import threading

import numpy as np
import pytest

from conftest import to_device
from resize_cases import SOURCE_COLUMNS, SOURCE_ROWS, source_frame
from test_gpu_resize_filters import HDRI, Q16, check, reference, resize

pytestmark = pytest.mark.gpu

PLANS_KEPT = 16
# (columns, row counts, the kernel that must take every call)
STREAM_WALK = (2 * SOURCE_COLUMNS, list(range(46, 64)), "resize_stream")
MATRIX_WALK = (85, list(range(53, 71)), "resize_mfma")


def walk_cases(walk):
    columns, row_counts, kernel = walk
    assert len(row_counts) > PLANS_KEPT and columns * (1.0 / SOURCE_COLUMNS) <= row_counts[0] * (1.0 / SOURCE_ROWS)
    return [((columns, rows), kernel) for rows in row_counts]


def frame(dtype):
    return source_frame(SOURCE_ROWS, SOURCE_COLUMNS, 4, dtype, True)


def want(refmod, px, target):
    return reference(refmod, ("plan caches",), px, True, target, "lanczos")


@pytest.mark.parametrize("walk", [STREAM_WALK, MATRIX_WALK], ids=["streaming", "matrix"])
@pytest.mark.parametrize("dtype", [Q16, HDRI], ids=["q16", "float"])
def test_more_plans_than_the_cache_keeps(im, refmod, dtype, walk):
    """18 geometries through a cache of 16, then the first two again: their plans were evicted and are rebuilt."""
    px = frame(dtype)
    cases = walk_cases(walk)
    for target, kernel in cases + cases[:2]:
        got, launched = resize(im, px, True, target, "lanczos", False)
        assert kernel in launched, (target, launched)
        check(got, want(refmod, px, target), px, False, "%s -> %dx%d %s" % (kernel, target[0], target[1], px.dtype.name))


def test_four_threads_share_the_plan_caches(im, refmod):
    """Four threads, each on its own stream, walk both forms' geometries (36: both caches overflow all the time) in
    different orders: a thread's plan may be evicted, and destroyed, by another thread while its kernel is queued."""
    import torch
    cases = walk_cases(STREAM_WALK) + walk_cases(MATRIX_WALK)
    frames = {dtype: frame(dtype) for dtype in (Q16, HDRI)}
    for px in frames.values():
        for target, _ in cases:
            want(refmod, px, target)                    # computed once, before the threads start
    results, errors = {}, []

    def work(k):
        try:
            px = frames[(Q16, HDRI)[k % 2]]
            order = np.random.default_rng(50 + k).permutation(len(cases))
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                image = im.Image(to_device(px), has_alpha=True, precision=im.PRECISION_FAST)
                for i in order:
                    target = cases[i][0]
                    out = im.resize_image(image, target[0], target[1], "lanczos")
                    stream.synchronize()
                    results[(k, target)] = out.numpy()
        except Exception as exc:                        # surfaced below
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 4 * len(cases)
    for (k, target), got in sorted(results.items()):
        px = frames[(Q16, HDRI)[k % 2]]
        check(got, want(refmod, px, target), px, False, "thread %d -> %dx%d %s" % (k, target[0], target[1], px.dtype.name))
