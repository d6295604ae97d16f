"""The index tables of a bundle-adjustment problem (easysfm_amd/csrc/ba_layout.cpp) are host-only code: tests/cpp/ba_layout_check.cpp
generates seeded observation lists and checks what the kernels rely on in them -- the point sort, the camera chunks, the three
families of Schur tables and the point chunks -- with g++ alone, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "ba_layout_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ba_layout_check.cpp"),
                        os.path.join(CSRC, "ba_layout.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ba layout ok" in r.stdout, r.stdout[-4000:]


def test_ba_layout_invariants(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_ba_layout_under_asan(tmp_path):
    """The same program with AddressSanitizer + UBSan (host code, CPU only): the table builders index a dozen arrays by each other."""
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
