"""The fused L2 launch's host arithmetic (easysfm_amd/csrc/match_plan.hpp: fused_grid_of, pair_blocks2) has no GPU dependency:
tests/cpp/match_fused_grid_check.cpp checks the padded pass count, the role boundary, the finish role's XCD alignment and that every
pair waits for exactly the pass blocks that name it -- on the degenerate lists of tests/test_match_fused_gpu.py, a list of
65 535-row train sets and seeded lists -- with g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "match_fused_grid_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "match_fused_grid_check.cpp"),
                        os.path.join(CSRC, "match_plan.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "fused grid ok" in r.stdout, r.stdout[-4000:]


def test_fused_grid_invariants(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_fused_grid_under_asan(tmp_path):
    """The same program with AddressSanitizer + UBSan (host code, CPU only)."""
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
