"""The kernels of threshold.hip are in the built library and keep everything in registers and LDS:
no scratch.  Read from the code objects' metadata (tools/kernel_resources.py); no GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_threshold_kernels_exist_and_do_not_spill():
    import kernel_resources
    if not os.path.exists(kernel_resources.DEFAULT_LIBRARY) or not os.path.exists(kernel_resources.OBJCOPY):
        pytest.skip("library or llvm-objcopy not present")
    kernels = kernel_resources.kernel_resources()
    # the pointwise and histogram kernels: two Quantum types x 1-4 channels; AdaptiveThresholdImage has
    # one kernel per Quantum type, x 1-4 channels
    for name, count in (("threshold_point_kernel<", 8), ("threshold_histogram_kernel<", 8),
                        ("adaptive_q16_kernel<", 4), ("adaptive_float_kernel<", 4)):
        rows = [k for k in kernels if name in k["name"]]
        assert len(rows) == count, (name, [k["name"] for k in rows])
        for k in rows:
            assert k["scratch"] == 0, k
