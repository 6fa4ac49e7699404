"""The generated inline assembly of zk-fhe_amd/csrc/mont29_tied.inc (mont29u_* / mont29i_*: mul_v, mul_s, sqr, mul2) run ON THE DEVICE at
the largest operands each wrapper's declared bound admits -- tests/native/tied_products_check.hip: one case list evaluated by a kernel,
by the host's C body and by the standard 8 x 32-bit arithmetic.  Built with the flags the library is built with, run once as a child
process.  The host half of the same file (C body against the reference) also runs without a GPU."""
import os
import shutil
import subprocess
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "tied_products_check.hip")


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


@pytest.fixture(scope="module")
def device_exe(tmp_path_factory):
    """compiled once per module, with zk_fhe_amd.build.FLAGS: -O3 and the unroll threshold decide what the assembly's surroundings look like"""
    from zk_fhe_amd import build
    exe = str(tmp_path_factory.mktemp("tied") / "tied_products_check")
    t0 = time.time()
    subprocess.run([_hipcc(), *build.FLAGS, "-I", build.CSRC, SRC, "-o", exe], check=True)
    print("tied_products_check: compiled in %.1f s" % (time.time() - t0))
    return exe


@pytest.mark.gpu
def test_tied_products_on_the_device_at_their_bounds(device_exe):
    """lz_mul (limb types (2,2), (1,2), (2,1)) at 160 r, lz_mul<true> (mont29i_mul_s) against a kernel-argument constant, lz_mul2 at 80 r
    twice, lz_mul4u, lq_mul / lq_sqr / lq_mul2 and the unsigned mul_v / sqr / mul2 of both fields at 11 p, lz_weak / lz_store on every
    multiple of r within 16 r and its neighbours, each against the largest canonical constant, p - 1, 0, 1 and random ones, plus
    300 random operands per product: device == host == reference, bit for bit."""
    r = subprocess.run([device_exe], capture_output=True, text=True, timeout=120)   # one launch of 29 blocks and five of 3: well under a second of GPU time
    assert r.returncode == 0 and "tied products: 0 bad" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    assert "device, host and reference" in r.stdout


def test_tied_products_case_list_on_the_host(tmp_path):
    """the same case list, host only: the C body (what -DZK_MAD_C also selects on the device) against the 8 x 32-bit reference.  A plain
    C++ build of the same file: no device pass, a few seconds."""
    exe = str(tmp_path / "tied_products_host")
    subprocess.run([_hipcc(), "-x", "c++", "-O2", "-std=c++17", "-DZK_MAD_C", "-I", os.path.join(ROOT, "zk-fhe_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tied products: 0 bad" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
