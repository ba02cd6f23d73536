"""ResizeImage's two separate passes (imagemagick_amd/csrc/resize.hip) read tables built on the host and launch with a
geometry worked out on the host (resize_pass_plan.hpp).  tests/cpu/resize_pass_plan_test.cpp builds contribution lists
for the geometries of tests/resize_cases.py — the ten tap cases, the wide Point reduction, the degenerate columns —,
for sizes that are no multiple of a tile and for a list with empty windows, and checks the vertical kernel's dense
weights, masks and widest tile, the horizontal kernel's spans, overhang and per-tile tap counts, and the kernel, rows and
LDS bytes chosen for every layout.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_tables_and_launch_geometry():
    exe = os.path.join(tempfile.mkdtemp(prefix="mh_pass_"), "pass_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "imagemagick_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "resize_pass_plan_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
