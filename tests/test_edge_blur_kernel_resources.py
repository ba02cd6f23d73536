"""The BilateralBlurImage and SelectiveBlurImage kernels (edge_blur.hip) are in the built library and
keep everything in registers and LDS: no scratch.  Read from the code objects' metadata
(tools/kernel_resources.py); no GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("kernel", ["bilateral_blur_kernel<", "selective_blur_kernel<"])
def test_edge_blur_kernels_exist_and_do_not_spill(kernel):
    import kernel_resources
    if not os.path.exists(kernel_resources.DEFAULT_LIBRARY) or not os.path.exists(kernel_resources.OBJCOPY):
        pytest.skip("library or llvm-objcopy not present")
    rows = [k for k in kernel_resources.kernel_resources() if kernel in k["name"]]
    # two Quantum types x four channel counts
    assert len(rows) == 8, [k["name"] for k in rows]
    for k in rows:
        assert k["scratch"] == 0, k
