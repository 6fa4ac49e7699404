"""csrc/ntt_plan.hpp on the CPU: the pass schedule and buffer routing of a long-row NTT call (tests/native/ntt_plan_check.cpp)."""
import os
import shutil
import subprocess

import pytest


def test_ntt_plan_schedule(tmp_path):
    """For every row length 2^14 .. 2^26, both directions, in place and out of place, with no coset, a device table of coset powers
    or host shifts, and ZKFHE_NTT_LDS_PASS on and off: the stages per pass equal a literal table taken from the former dispatcher's
    loop and sum to log_n - 13, only the first pass carries the coset multiplier, an LDS pass has 4 .. 6 stages, the four-step pass
    appears only at 2^16 and 2^19 with at most four rows and no table, the source is never written, the tile stage never reads the
    buffer it writes, a copy back follows exactly when the call is in place, and host shifts anywhere else are refused -- under the
    address and undefined-behaviour sanitizers.  The program is stand-alone: nothing is preloaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "zk-fhe_amd", "csrc")
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++")
    exe = str(tmp_path / "ntt_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                    os.path.join(here, "native", "ntt_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntt plan check: ok" in out.stdout, out.stdout + out.stderr
