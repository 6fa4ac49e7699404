"""host/chain_jobs.hpp on the CPU: the job list of a round's linear combinations (tests/native/chain_jobs_check.cpp), and the driver of
tests/test_gpu_chain_side_by_side.py compiled for gfx950."""
import os
import shutil
import subprocess
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "zk-fhe_amd", "host")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_chain_job_list(tmp_path, sanitize):
    """Member counts 1, 47, 48, 49, 96, 97 in 1, 6 and 8 sets, alone and mixed: every member in exactly one job of at most 48, one
    writer per destination row, partial slots used once and inside the partial-sum buffer of a k = 13 workspace.  Built plain and
    under the address and undefined-behaviour sanitizers; the program is stand-alone: nothing is preloaded."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++")
    exe = str(tmp_path / "chain_jobs_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", HOST, os.path.join(HERE, "native", "chain_jobs_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_side_by_side_driver_compiles_for_gfx950(tmp_path):
    """compile only: the device pass for gfx950 with the library's flags, no link, nothing run"""
    from zk_fhe_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    t0 = time.time()
    subprocess.run([hipcc, *build.FLAGS, "-I", HOST, "-I", build.CSRC, "-c", os.path.join(HERE, "native", "chain_side_by_side_driver.hip"), "-o", str(tmp_path / "driver.o")],
                   check=True)
    print("chain_side_by_side_driver: compiled in %.1f s" % (time.time() - t0))
