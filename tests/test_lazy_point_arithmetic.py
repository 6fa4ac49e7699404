"""The lazy signed-limb arithmetic over Fq and the point operations of the MSM kernels written on it (zk-fhe_amd/csrc/fq29.hip.hpp:
Lz<LO, HI, V>, lq_mul / lq_sqr / lq_mul2, g1x29_add_affine / g1x29_add / g1x29_dbl) against the 8 x 32-bit arithmetic of
bn254.hip.hpp.  The code is host+device; this builds and runs its host instantiation (the C bodies of the products, which
-DZK_MAD_C also selects on the device) -- no GPU.  The generated assembly the device runs instead (csrc/mont29_tied.inc) meets the
same extreme operands in tests/test_gpu_tied_products.py; tests/test_gpu_msm_lazy.py reaches it only through whole MSMs on random
scalars, which stay far below the bounds."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build(tmp_path, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "lq29_check")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", *extra, "-I", os.path.join(ROOT, "zk-fhe_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "native", "lq29_check.hip"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("flags", [(), ("-DZK_MAD_C",)], ids=["default", "ZK_MAD_C"])
def test_lazy_fq_products_and_point_operations(tmp_path, flags):
    """Bit for bit after canonicalisation: the products on random operands, on 0, 1, p - 1 and on the largest values of either sign
    each declared bound admits; the zero test on every multiple of p its bound admits; the three point operations on random points,
    the generator, an empty accumulator, an identity entry, Q = P (doubling) and Q = -P (cancellation) with either sign flag, and on the
    extreme representatives of an accumulator (x up to +-8 p, y, zz, zzz down to -p); one chain of 12 000 mixed additions into one
    accumulator with no canonicalisation in between, its limbs inside the declared bounds after every addition."""
    out = subprocess.run([_build(tmp_path, flags)], check=True, capture_output=True, text=True).stdout
    assert "lq29: 0 bad" in out, out
