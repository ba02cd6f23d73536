"""SampleImage, ScaleImage and ThumbnailImage through the HIP-backed MagickCore: the shim's hooks in front
of the sized CloneImage of SampleImage and ScaleImage send the call to libmagickhip.so, ThumbnailImage
becomes resident because its three callees are, and every result is the pure-CPU one - in a process of its
own where nothing sets the precision, so the library runs in its default FAST mode
(tests/scale_shim_child.py).  A call the hook's gate declines is left to MagickCore."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = (b"MagickHipSampleImage\0", b"MagickHipScaleImage\0")


def has_scale_hooks(refmod, hdri):
    """A HIP-backed MagickCore linked before these hooks existed resolves neither entry point
    (shim/opencl_hip.c): its SampleImage and ScaleImage run MagickCore's own code."""
    with open(refmod.shim_lib_path(hdri), "rb") as f:
        data = f.read()
    return all(name in data for name in HOOKS)


@pytest.fixture(scope="module")
def report(refmod, im):
    if not (os.path.exists(refmod.shim_lib_path(False)) and os.path.exists(refmod.shim_lib_path(True))):
        pytest.skip("the HIP-backed MagickCore (oracle/_ref/libMagickCore-hip-*.so) is not built")
    if not (has_scale_hooks(refmod, False) and has_scale_hooks(refmod, True)):
        pytest.skip("the HIP-backed MagickCore in oracle/_ref predates the scale hooks (rebuild: make -C shim)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MAGICKHIP_") and k != "MAGICK_HIP_PRECISION"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scale_shim_child.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_the_process_ran_in_the_default_mode(report):
    assert report["precision"] == 1, "the library's default is FAST"


@pytest.mark.parametrize("operator", ["sample", "scale"])
def test_through_magickcore_is_the_cpu_result(report, operator):
    assert len(report[operator]) >= 3
    for case in report[operator]:
        assert case["accelerated"] == 1, "%s did not take the accelerated path as one call: %s" % (operator, case)
        assert case["differing"] == 0, "%s via MagickCore differs from the reference: %s" % (operator, case)
        assert case["type"] == case["cpu_type"], case


def test_a_thumbnail_is_the_cpu_result_and_stays_on_the_device(report):
    assert len(report["thumbnail"]) == 6
    for case in report["thumbnail"]:
        assert case["accelerated"] == case["stages"], case          # one count per hooked callee
        assert case["differing"] == 0, "ThumbnailImage via MagickCore differs from the reference: %s" % case
        assert case["type"] == case["cpu_type"], case
        # one upload of the source, nothing until the thumbnail is read, then its one download
        assert (case["uploads"], case["downloads_before_the_read"]) == (1, 0), case
        assert (case["uploads_after_the_read"], case["downloads"]) == (1, 1), case


def test_the_profile_records_show_the_device_ran(report):
    for kernel in ("sample", "scale_fused", "scale_rows", "scale_columns", "resize_vertical", "resize_horizontal"):
        assert kernel in report["kernels"], report["kernels"]


def test_calls_in_front_of_the_hook_or_declined_by_the_gate_are_the_cpu_result(report):
    assert len(report["masked"]) == 6                     # a read mask on a Q16 and on a float frame, three calls each
    for case in report["identity"] + report["declined"] + report["masked"]:
        assert case["accelerated"] == 0 and case["differing"] == 0, case
    # a write- or composite-masked frame: the reference's own result is not reproducible
    # (tests/scale_shim_child.py); the path and the geometry
    assert len(report["unset_masked"]) == 4
    for case in report["unset_masked"]:
        assert case["accelerated"] == 0 and case["differing"] >= 0, case
