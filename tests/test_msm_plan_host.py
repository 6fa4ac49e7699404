"""csrc/msm_plan.hpp on the CPU: the geometry and scratch layout of a bucket-pipeline MSM call (tests/native/msm_plan_check.cpp)."""
import os
import shutil
import subprocess

import pytest


def test_msm_plan_layout(tmp_path):
    """Every array of a call lies inside its scratch slot, live arrays do not overlap, the aliases lie inside what they alias, the
    alignments the kernels rely on hold, and geometry and slot sizes equal the dispatcher's former formulas -- for twelve call
    geometries (K < 64 to K = 32768, one to 4096 columns, every ZKFHE_SORT mode), under the address and undefined-behaviour
    sanitizers.  The program is stand-alone: nothing is preloaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "zk-fhe_amd", "csrc")
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++")
    exe = str(tmp_path / "msm_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                    os.path.join(here, "native", "msm_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "msm plan check: ok" in out.stdout, out.stdout + out.stderr
