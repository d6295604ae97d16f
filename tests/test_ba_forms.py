"""Which form of the size-dependent bundle-adjustment kernels a problem takes (easysfm_amd/csrc/ba_forms.cpp) is host-only
arithmetic: tests/cpp/ba_forms_check.cpp asserts the table of DESIGN.md section 5.1a at every boundary and its neighbour, and over
every accepted camera count, with g++ alone, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")


def test_ba_forms_table(tmp_path):
    exe = str(tmp_path / "ba_forms_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_forms_check.cpp"),
                        os.path.join(CSRC, "ba_forms.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ba forms ok" in r.stdout, r.stdout[-4000:]
