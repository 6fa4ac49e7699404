"""The kernels of zk-fhe_amd/host/prover_kernels.hip.hpp alone, against Python integers: the permutation and lookup numerators and
denominators, the running products (one workgroup per column and in segments) and their chunk carries, the barycentric evaluations, the
SHPLONK linear combinations and quotients, the quotient combination and the small element-wise kernels -- at the operand extremes, the
shapes and the grand products that an honest proof never shows, and with every row a kernel has to leave alone checked for the
sentinel it started with.  tests/native/prover_kernels_driver.hip launches them with the prover's block sizes on the case list of
tests/prover_kernel_cases.py: compiled once with the library's flags, run once as a child process; the tests only compare arrays.
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import os
import shutil
import subprocess
import time

import pytest

from tests import prover_kernel_cases as pc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "prover_kernels_driver.hip")


def compile_driver(exe):
    from zk_fhe_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    host = os.path.join(ROOT, "zk-fhe_amd", "host")
    t0 = time.time()
    subprocess.run([hipcc, *build.FLAGS, "-I", host, "-I", build.CSRC, SRC, "-o", exe], check=True)
    print("prover_kernels_driver: compiled in %.1f s" % (time.time() - t0))
    return exe


def write_cases(d):
    c = pc.build()
    os.makedirs(os.path.join(d, "in"))
    os.makedirs(os.path.join(d, "out"))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write(c.text())
    for name, data in c.files.items():
        with open(os.path.join(d, "in", name), "wb") as f:
            f.write(data)
    return c


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """the driver's one run: some 330 cases, a few hundred launches of well under a second of kernel time together; the rest is process
    start, 120 MB of input files and 290 MB of output files.  Measured 0.4 s on an MI355X box (the compile before it: half a minute);
    the limit of 60 s covers that step alone and leaves room for a slow disk."""
    exe = compile_driver(str(tmp_path_factory.mktemp("pk_exe") / "prover_kernels_driver"))
    d = str(tmp_path_factory.mktemp("pk_cases"))
    c = write_cases(d)
    t0 = time.time()
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=60)
    print("prover_kernels_driver: ran in %.1f s: %s" % (time.time() - t0, r.stdout.strip()[-200:]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d cases run" % sum(l.startswith("run ") for l in c.lines) in r.stdout

    def read(buf):
        with open(os.path.join(d, "out", buf + ".bin"), "rb") as f:
            return f.read()
    yield c, read
    shutil.rmtree(d, ignore_errors=True)   # 400 MB of arrays


@pytest.mark.parametrize("group", pc.GROUPS)
def test_prover_kernels_against_python_integers(outputs, group):
    """every output word of the group's cases, bit for bit; untouched rows still hold the sentinel"""
    c, read = outputs
    bad = pc.mismatches(c, group, read)
    assert not bad, "%d of %d arrays differ:\n%s" % (len(bad), len(c.checks[group]), "\n".join(bad[:20]))
