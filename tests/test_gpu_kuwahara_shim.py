"""KuwaharaImage through the HIP-backed MagickCore: the shim's hook in front of the operator's
BlurImage (effect.c:1810) sends the whole call to libmagickhip.so, and the result is the pure-CPU one
bit for bit - in a process of its own where nothing sets the precision, so the library runs in its
default FAST mode (tests/kuwahara_shim_child.py).  An interpolation method the library does not
restate is left to MagickCore's CPU code."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def has_kuwahara_hook(refmod, hdri):
    """A HIP-backed MagickCore linked before this hook existed resolves no MagickHipKuwaharaImage
    (shim/opencl_hip.c): its KuwaharaImage runs MagickCore's own code behind the accelerated BlurImage."""
    with open(refmod.shim_lib_path(hdri), "rb") as f:
        return b"MagickHipKuwaharaImage\0" in f.read()


@pytest.fixture(scope="module")
def report(refmod, im):
    if not (os.path.exists(refmod.shim_lib_path(False)) and os.path.exists(refmod.shim_lib_path(True))):
        pytest.skip("the HIP-backed MagickCore (oracle/_ref/libMagickCore-hip-*.so) is not built")
    if not (has_kuwahara_hook(refmod, False) and has_kuwahara_hook(refmod, True)):
        pytest.skip("the HIP-backed MagickCore in oracle/_ref predates the KuwaharaImage hook (rebuild: make -C shim)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MAGICKHIP_") and k != "MAGICK_HIP_PRECISION"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kuwahara_shim_child.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_the_process_ran_in_the_default_mode(report):
    assert report["precision"] == 1, "the library's default is FAST"


def test_kuwahara_through_magickcore_moves_the_counter(report):
    assert len(report["cases"]) == 10
    for case in report["cases"]:
        assert case["accelerated"] == 1, "KuwaharaImage did not take the accelerated path: %s" % case


def test_kuwahara_through_magickcore_is_the_cpu_result(report):
    for case in report["cases"]:
        assert case["changed"] > 0, case
        assert case["differing"] == 0, "KuwaharaImage via MagickCore differs from the reference: %s" % case


@pytest.mark.parametrize("quantum", ["uint16", "float32"])
def test_nearest_interpolation_is_left_to_the_cpu(report, quantum):
    r = report["nearest_" + quantum]
    assert r["accelerated"] == 0, "a Nearest-interpolation call was accelerated"
    assert r["differing"] == 0
    assert r["differs_from_bilinear"] > 0, "Nearest gives the bilinear result: the case tests nothing"


def test_a_declined_call_is_the_cpu_result_blur_included(report):
    """A declined KuwaharaImage keeps its BlurImage on the CPU as well: behind a blur that is only
    within one level the selection would not be the CPU's."""
    r = report["over_the_limit"]
    assert r["accelerated"] == 0 and r["differing"] == 0, r
