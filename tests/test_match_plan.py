"""The pair plan of the matchers (easysfm_amd/csrc/match_plan.cpp) is host-only code shared by the plain and the guided matcher:
tests/cpp/match_plan_check.cpp generates seeded set sizes and pair lists and checks what the kernels rely on in its tables -- the
prefix sums, the two workgroup numberings, the front pass's block table, the pair order by train set, the mirrored half of the
cross-check -- and that either rule set refuses the sizes it refuses with the messages it has, with g++ alone, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "easysfm_amd", "csrc")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "match_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "match_plan_check.cpp"),
                        os.path.join(CSRC, "match_plan.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "match plan ok" in r.stdout, r.stdout[-4000:]


def test_match_plan_invariants(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_match_plan_under_asan(tmp_path):
    """The same program with AddressSanitizer + UBSan (host code, CPU only)."""
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
