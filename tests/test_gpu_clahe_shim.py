"""CLAHEImage through the HIP-backed MagickCore: the shim's hook at the top of the operator sends the
whole call, both colourspace transforms included, to libmagickhip.so, and the result is the pure-CPU
one bit for bit - in a process of its own where nothing sets the precision, so the library runs in
its default FAST mode (tests/clahe_shim_child.py).  A frame the library declines is left to
MagickCore's CPU code, transforms included."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def has_clahe_hook(refmod, hdri):
    """A HIP-backed MagickCore linked before this hook existed resolves no MagickHipCLAHEImage
    (shim/opencl_hip.c): its CLAHEImage runs MagickCore's own code between accelerated transforms."""
    with open(refmod.shim_lib_path(hdri), "rb") as f:
        return b"MagickHipCLAHEImage\0" in f.read()


@pytest.fixture(scope="module")
def report(refmod, im):
    if not (os.path.exists(refmod.shim_lib_path(False)) and os.path.exists(refmod.shim_lib_path(True))):
        pytest.skip("the HIP-backed MagickCore (oracle/_ref/libMagickCore-hip-*.so) is not built")
    if not (has_clahe_hook(refmod, False) and has_clahe_hook(refmod, True)):
        pytest.skip("the HIP-backed MagickCore in oracle/_ref predates the CLAHEImage hook (rebuild: make -C shim)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MAGICKHIP_") and k != "MAGICK_HIP_PRECISION"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "clahe_shim_child.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_the_process_ran_in_the_default_mode(report):
    assert report["precision"] == 1, "the library's default is FAST"


def test_clahe_through_magickcore_moves_the_counter(report):
    assert len(report["cases"]) == 3
    for case in report["cases"] + [report["lab"]]:
        assert case["accelerated"] == 1, "CLAHEImage did not take the accelerated path as one call: %s" % case


def test_clahe_through_magickcore_is_the_cpu_result(report):
    for case in report["cases"] + [report["lab"]]:
        assert case["changed"] > 0, case
        assert case["differing"] == 0, "CLAHEImage via MagickCore differs from the reference: %s" % case
        assert case["colorspace"] == case["cpu_colorspace"]


def test_a_gray_frame_is_left_to_the_cpu(report):
    r = report["gray"]
    assert r["accelerated"] == 0 and r["differing"] == 0 and r["changed"] > 0, r


def test_a_call_the_library_declines_is_the_cpu_result_transforms_included(report):
    r = report["table"]
    assert r["accelerated"] == 0 and r["differing"] == 0 and r["changed"] > 0, r
