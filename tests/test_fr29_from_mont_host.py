"""tests/native/fr29_from_mont_check.hip: fr29_from_mont_weak (zk-fhe_amd/csrc/fr29.hip.hpp) -- a scalar out of Montgomery form by one
nine-limb reduction of 32 x, as the table MSM takes it -- against the 8 x 32-bit fp_from_mont, as a stand-alone host program built once
plain and once with the undefined-behaviour and address sanitizers on the host pass.  Host instantiation of the host+device code (no GPU)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("sanitize", [False, True])
def test_nine_limb_conversion_against_the_standard_one(tmp_path, sanitize):
    """0, the multiples of r below 2^256 (r, not 0, for the non-zero ones: the sign split of the MSM sends both to magnitude 0) and
    their neighbours, 2^256 - 1, and 200 000 random words with and without whole limbs of zeros or ones"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "fr29_from_mont_check")
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([hipcc] + flags + ["-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "zk-fhe_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "native", "fr29_from_mont_check.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fr29_from_mont_weak: 0 bad, r for 5 inputs" in r.stdout, r.stdout + r.stderr
