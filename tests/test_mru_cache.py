"""The resize launchers keep their contribution tables, device tables and plans in small most-recently-used caches
(imagemagick_amd/csrc/mru_cache.hpp).  tests/cpu/mru_cache_test.cpp drives one with a counting value: a hit moves to
the front, the least recently used entry leaves a full cache, what leaves is destroyed by the caller and never inside
insert() or clear() (a plan's destructor waits for the device), two builders of one key leave one entry, and four
threads over three times the capacity in keys end with a full cache whose every live value is found.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mru_cache_hands_out_what_it_evicts():
    exe = os.path.join(tempfile.mkdtemp(prefix="mh_mru_"), "mru_cache_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "imagemagick_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "mru_cache_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
