"""csrc/g1_fft_plan.hpp and csrc/g1_fft_ladder.hip.hpp on the CPU (tests/native/g1_fft_plan_check.cpp), and the header side of
the ceremony calls: the new constants against the Python module, the new declarations."""
import os
import re
import shutil
import subprocess

import pytest

import zk_fhe_amd as zk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_g1_fft_schedule_against_naive_sum(tmp_path):
    """The schedule and the butterfly arithmetic of zkfhe_g1_fft, walked on the host for every log_n from 1 to 6, both directions,
    over random points and the degenerate inputs (all G, w^j G, all identity, identity at the odd indices, one point alone), in the
    window structure (what the launcher picks below 2^7) and, through a narrower wave, in the shared-twiddle structure: byte for
    byte the naive double sum.  Also: every slot is touched once per stage, the lanes of a wave share a twiddle, and what
    k_g1_fft_shared relies on holds for every size up to 2^20.  Stand-alone program under the address and undefined-behaviour
    sanitizers; nothing is preloaded."""
    csrc = os.path.join(ROOT, "zk-fhe_amd", "csrc")
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++")
    exe = str(tmp_path / "g1_fft_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                    os.path.join(HERE, "native", "g1_fft_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "g1 fft plan check: ok" in out.stdout, out.stdout + out.stderr


def _header():
    return open(os.path.join(ROOT, "include", "zkfhe.h")).read()


def test_header_constants_match_python():
    defs = dict(re.findall(r"#define\s+(ZKFHE_[A-Z0-9_]+)\s+(-?\d+)\b", _header()))
    assert int(defs["ZKFHE_PROF_G1_FFT"]) == zk.PROF_G1_FFT == 23
    assert int(defs["ZKFHE_SRS_BAD_POWERS"]) == zk.SRS_BAD_POWERS == 1
    assert int(defs["ZKFHE_SRS_BAD_LAGRANGE"]) == zk.SRS_BAD_LAGRANGE == 2
    assert int(defs["ZKFHE_SRS_BAD_GENERATOR"]) == zk.SRS_BAD_GENERATOR == 4


def test_ceremony_calls_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = zk.load_library()
    for name in ("zkfhe_g1_fft", "zkfhe_srs_from_monomial", "zkfhe_srs_load_downsized", "zkfhe_srs_check"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in zk.EXPORTS and hasattr(lib, name), name
    for name in ("g1_fft",):
        assert hasattr(zk.Context, name)
    for name in ("from_monomial", "load_downsized", "check"):
        assert hasattr(zk.Srs, name)


def test_launcher_switch_size_is_what_the_gpu_test_names():
    """tests/test_gpu_g1_fft.py names log_n = 6 and 7 as the two sides of the one switch between kernel structures: the first stage
    of 2^7 points is the first with a wave's worth of blocks."""
    plan = open(os.path.join(ROOT, "zk-fhe_amd", "csrc", "g1_fft_plan.hpp")).read()
    wave = int(re.search(r"constexpr int G1FFT_WAVE = (\d+);", plan).group(1))
    first = int(re.search(r"constexpr int G1FFT_FIRST_SHARED_LOG = (\d+);", plan).group(1))
    assert wave == 64 and first == 7 and 1 << (first - 1) == wave
