"""tests/native/fr9_check.hip: the nine-limb Fr value of the quotient, lookup, scan and batch-inversion kernels
(zk-fhe_amd/csrc/fr9.hip.hpp) against the standard 8 x 32-bit Fr arithmetic, as a stand-alone host program -- built once plain and
once with the undefined-behaviour and address sanitizers on the host pass.  Host instantiation of the same host+device code (no GPU)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("sanitize", [False, True])
def test_nine_limb_fr_value_against_the_standard_arithmetic(tmp_path, sanitize):
    """both loads, the regrouping by five bits, fr9_mul / fr9_sqr / fr9_mul2 at the extreme members of every bound they declare, the
    canonical store, and v + b s + g, z1 A - z0 B, the Horner steps and the inversion chains as the kernels write them, on random
    operands and on every combination of 0, 1, r - 1, r - 2, 2^253, 2^253 - 1 and the limb-wise largest canonical word"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "fr9_check")
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([hipcc] + flags + ["-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "zk-fhe_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "native", "fr9_check.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fr9: 0 bad" in r.stdout and "fr9 edges: 0 bad" in r.stdout, r.stdout + r.stderr
