"""host/workspace_layout.hpp on the CPU: the prover workspace's sizes and named regions (tests/native/workspace_layout_check.cpp)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "zk-fhe_amd", "host")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_workspace_layout(tmp_path, sanitize):
    """Toy, k = 13, k = 16, k = 19 and the widest admissible shape, with 3 and 4 coset rows: the layout is consistent, every accessor's
    region is one of the table's, the totals are the earlier allocation formulas' less exactly the dropped buffers; two same-step regions
    made to overlap are reported.  Built plain and under the address and undefined-behaviour sanitizers; the program is stand-alone:
    nothing is preloaded."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++")
    exe = str(tmp_path / "workspace_layout_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", HOST, os.path.join(HERE, "native", "workspace_layout_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
