"""The KuwaharaImage kernel (kuwahara.hip) is in the built library and keeps everything in registers
and LDS: no scratch.  Read from the code objects' metadata (tools/kernel_resources.py); no GPU
needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_kuwahara_kernels_exist_and_do_not_spill():
    import kernel_resources
    if not os.path.exists(kernel_resources.DEFAULT_LIBRARY) or not os.path.exists(kernel_resources.OBJCOPY):
        pytest.skip("library or llvm-objcopy not present")
    rows = [k for k in kernel_resources.kernel_resources() if "kuwahara_kernel<" in k["name"]]
    # two Quantum types x four channel counts
    assert len(rows) == 8, [k["name"] for k in rows]
    for k in rows:
        assert k["scratch"] == 0, k
