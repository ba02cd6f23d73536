"""AdaptiveThresholdImage, BilevelImage and AutoThresholdImage through the HIP-backed MagickCore: the
shim's hooks at the top of the three operators send the call to libmagickhip.so, and the result, the
colourspace and the auto-threshold:threshold property are the pure-CPU ones - in a process of its own
where nothing sets the precision, so the library runs in its default FAST mode
(tests/threshold_shim_child.py).  A call the hook or the library declines is left to MagickCore."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = (b"MagickHipBilevelImage\0", b"MagickHipAutoThresholdImage\0", b"MagickHipAdaptiveThresholdImage\0")


def has_threshold_hooks(refmod, hdri):
    """A HIP-backed MagickCore linked before these hooks existed resolves none of the three entry
    points (shim/opencl_hip.c): its threshold operators run MagickCore's own code."""
    with open(refmod.shim_lib_path(hdri), "rb") as f:
        data = f.read()
    return all(name in data for name in HOOKS)


@pytest.fixture(scope="module")
def report(refmod, im):
    if not (os.path.exists(refmod.shim_lib_path(False)) and os.path.exists(refmod.shim_lib_path(True))):
        pytest.skip("the HIP-backed MagickCore (oracle/_ref/libMagickCore-hip-*.so) is not built")
    if not (has_threshold_hooks(refmod, False) and has_threshold_hooks(refmod, True)):
        pytest.skip("the HIP-backed MagickCore in oracle/_ref predates the threshold hooks (rebuild: make -C shim)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MAGICKHIP_") and k != "MAGICK_HIP_PRECISION"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "threshold_shim_child.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_the_process_ran_in_the_default_mode(report):
    assert report["precision"] == 1, "the library's default is FAST"


@pytest.mark.parametrize("operator", ["adaptive", "bilevel", "auto"])
def test_through_magickcore_is_the_cpu_result(report, operator):
    assert len(report[operator]) == 3
    for case in report[operator]:
        assert case["accelerated"] == 1, "%s did not take the accelerated path as one call: %s" % (operator, case)
        assert case["changed"] > 0, case
        assert case["differing"] == 0, "%s via MagickCore differs from the reference: %s" % (operator, case)
        assert case["colorspace"] == case["cpu_colorspace"], case


def test_the_property_string_is_the_reference_s(report):
    for case in report["auto"]:
        assert case["cpu_property"] is not None and case["cpu_property"].endswith("%"), case
        assert case["property"] == case["cpu_property"], case


def test_the_profile_records_show_the_device_ran(report):
    for kernel in ("adaptive_threshold_q16", "adaptive_threshold_float", "threshold_bilevel", "threshold_histogram"):
        assert kernel in report["kernels"], report["kernels"]


def test_calls_the_library_or_the_gate_declines_are_the_cpu_result(report):
    for name in ("wide", "tile"):
        r = report[name]
        assert r["accelerated"] == 0 and r["differing"] == 0 and r["changed"] > 0, (name, r)
