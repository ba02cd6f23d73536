"""The kernels of scale.hip are in the built library, for both Quantum types and 1-4 channels, and keep
everything in registers and LDS: no scratch.  Read from the code objects' metadata
(tools/kernel_resources.py); no GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_scale_kernels_exist_and_do_not_spill():
    import kernel_resources
    if not os.path.exists(kernel_resources.DEFAULT_LIBRARY) or not os.path.exists(kernel_resources.OBJCOPY):
        pytest.skip("library or llvm-objcopy not present")
    kernels = kernel_resources.kernel_resources()
    # the one-launch ScaleImage, its two-launch generic form and SampleImage: two Quantum types x 1-4 channels
    for name in ("scale_fused_kernel<", "scale_rows_kernel<", "scale_columns_kernel<", "sample_kernel<"):
        rows = [k for k in kernels if name in k["name"]]
        assert len(rows) == 8, (name, [k["name"] for k in rows])
        for k in rows:
            assert k["scratch"] == 0, k
