"""The kernels of levels.hip are in the built library, for both Quantum types and 1-4 channels, and keep
everything in registers and LDS: no scratch.  Read from the code objects' metadata
(tools/kernel_resources.py); no GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_levels_kernels_exist_and_do_not_spill():
    import kernel_resources
    if not os.path.exists(kernel_resources.DEFAULT_LIBRARY) or not os.path.exists(kernel_resources.OBJCOPY):
        pytest.skip("library or llvm-objcopy not present")
    kernels = kernel_resources.kernel_resources()
    # the point and range kernels: two Quantum types x 1-4 channels; one kernel folds the range's partials
    for name, count in (("levels_point_kernel<", 8), ("levels_range_kernel<", 8), ("levels_range_finish_kernel", 1)):
        rows = [k for k in kernels if name in k["name"]]
        assert len(rows) == count, (name, [k["name"] for k in rows])
        for k in rows:
            assert k["scratch"] == 0, k
