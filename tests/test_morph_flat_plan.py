"""The flat Erode / Dilate kernels (imagemagick_amd/csrc/morphology_flat.hip) are routed and fed from tables built on
the host (morph_flat_plan.hpp).  tests/cpu/morph_flat_plan_test.cpp builds cell lists — Disk 1..15 and 31, Square,
Diamond, Octagon, Plus, off-centre rectangles, one-sided shapes, a gap, a shifted run — and checks that the rectangles
of widen/reach cover exactly the cells, that the convex levels list every kernel row once under its own half-width,
and that rects_takes() answers as the kernel's conditions state for 4-, 8- and 16-byte pixels.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_tables_describe_the_cells():
    exe = os.path.join(tempfile.mkdtemp(prefix="mh_flat_"), "flat_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "imagemagick_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "morph_flat_plan_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
