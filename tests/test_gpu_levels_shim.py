"""LevelImage, LevelizeImage, GammaImage, NegateImage, SigmoidalContrastImage, LinearStretchImage and
MinMaxStretchImage through the HIP-backed MagickCore: the shim's hooks at the top of the seven operators
send the call to libmagickhip.so, and the result, image->gamma and the histogram:linear-stretch property
are the pure-CPU ones - in a process of its own where nothing sets the precision, so the library runs in
its default FAST mode (tests/levels_shim_child.py).  A call the hook's gate declines is left to MagickCore.
The frames are Q16 wherever the curve calls libm, so every comparison is bit for bit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = (b"MagickHipLevelImage\0", b"MagickHipLevelizeImage\0", b"MagickHipGammaImage\0", b"MagickHipNegateImage\0",
         b"MagickHipSigmoidalContrastImage\0", b"MagickHipMinMaxStretchImage\0", b"MagickHipLinearStretchImage\0")
OPERATORS = ["level", "levelize", "gamma", "negate", "sigmoidal", "linear", "minmax"]


def has_levels_hooks(refmod, hdri):
    """A HIP-backed MagickCore linked before these hooks existed resolves none of the entry points
    (shim/opencl_hip.c): its level operators run MagickCore's own code."""
    with open(refmod.shim_lib_path(hdri), "rb") as f:
        data = f.read()
    return all(name in data for name in HOOKS)


@pytest.fixture(scope="module")
def report(refmod, im):
    if not (os.path.exists(refmod.shim_lib_path(False)) and os.path.exists(refmod.shim_lib_path(True))):
        pytest.skip("the HIP-backed MagickCore (oracle/_ref/libMagickCore-hip-*.so) is not built")
    if not (has_levels_hooks(refmod, False) and has_levels_hooks(refmod, True)):
        pytest.skip("the HIP-backed MagickCore in oracle/_ref predates the level hooks (rebuild: make -C shim)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MAGICKHIP_") and k != "MAGICK_HIP_PRECISION"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "levels_shim_child.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_the_process_ran_in_the_default_mode(report):
    assert report["precision"] == 1, "the library's default is FAST"


@pytest.mark.parametrize("operator", OPERATORS)
def test_through_magickcore_is_the_cpu_result(report, operator):
    assert len(report[operator]) == 3
    for case in report[operator]:
        assert case["accelerated"] == 1, "%s did not take the accelerated path as one call: %s" % (operator, case)
        assert case["changed"] > 0, case
        assert case["differing"] == 0, "%s via MagickCore differs from the reference: %s" % (operator, case)
        assert case["gamma"] == case["cpu_gamma"], case


def test_gamma_image_multiplies_the_image_gamma(report):
    first = report["gamma"][0]                    # sRGB, image->gamma 1/2.2, GammaImage(2.2)
    assert first["gamma"] == first["cpu_gamma"] and float(first["gamma"]) == pytest.approx(1.0)
    for case in report["level"] + report["negate"]:
        assert case["gamma"] == case["cpu_gamma"]


def test_the_property_string_is_the_reference_s(report):
    for case in report["linear"]:
        assert case["cpu_property"] is not None and case["cpu_property"].endswith("%"), case
        assert case["property"] == case["cpu_property"], case


def test_the_profile_records_show_the_device_ran(report):
    for kernel in ("levels_level", "levels_level_table", "levels_levelize", "levels_levelize_table", "levels_gamma_table",
                   "levels_negate", "levels_negate_gray", "levels_sigmoidal_table", "levels_range"):
        assert kernel in report["kernels"], report["kernels"]


def test_calls_in_front_of_the_hook_or_declined_by_the_gate_are_the_cpu_result(report):
    for case in report["identity"]:
        assert case["accelerated"] == 0 and case["differing"] == 0 and case["changed"] == 0, case
        assert case["gamma"] == case["cpu_gamma"], case
    for case in report["masked"]:
        assert case["accelerated"] == 0 and case["differing"] == 0 and case["changed"] > 0, case
