"""The prover's own NTT path, which the C API does not reach: zk_coset_ntt_rows (the first `rows` cosets of an extension, fewer than
2^lef of them, written densely) and zk_extend_lagrange (Lagrange columns -> coefficients -> coset rows), bit for bit against the CPU
oracle, at tile sizes below 2^13 and at the row lengths that take a table of coset powers -- whole proofs (k = 13, 14, 16, 19) never
run those.  tests/native/ntt_rows_driver.hip makes the calls: compiled once with the library's flags, linked against the built
library, run once as a child process; the tests only compare arrays.
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref
from tests.test_gpu_ntt_edges import COSET_PATTERNS, batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ntt_rows_driver.hip")
GUARD = 4096   # bytes of 0xA5 behind every output buffer

# (log_n, lef, rows): what the shape reaches
SHAPES = [
    (8, 2, 3),    # a small tile, fewer rows than cosets
    (13, 2, 3),   # zk_pre13
    (13, 1, 1),   # zk_pre13, one row
    (14, 2, 3),   # a single radix-2 stage with the table of coset powers
    (15, 2, 3),   # k_dif_fused<2> with the table
    (16, 2, 3),   # the four-step pass with shifts
    (16, 3, 5),   # a four-step size forced onto the table: more than four rows
    (17, 2, 3),   # the LDS pass with the table
]
COLUMNS = COSET_PATTERNS + ("random",)   # the structured columns of the coset tests and one random column


def name(shape):
    return "n%d_e%d_r%d" % shape


_columns = {}


def columns(log_n):
    """(4, n, 4): the same columns serve as coefficients (zk_coset_ntt_rows) and as Lagrange values (zk_extend_lagrange)"""
    if log_n not in _columns:
        pats, a = batch(log_n, only=COLUMNS)
        assert sorted(p[0] for p in pats) == sorted(COLUMNS)
        _columns[log_n] = a
    return _columns[log_n]


def compile_driver(exe):
    from zk_fhe_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    t0 = time.time()
    subprocess.run([hipcc, *build.FLAGS, "-I", build.CSRC, SRC, "-o", exe, "-L" + build.HERE, "-lzkfhe_hip", "-Wl,-rpath," + build.HERE], check=True)
    print("ntt_rows_driver: compiled in %.1f s" % (time.time() - t0))
    return exe


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """the driver's one run: sixteen calls on rows of at most 2^17 points and 0.3 GB of output files.  Measured 0.7 s on an MI355X box
    (the compile before it: one second); the limit of 60 s covers that step alone, context creation and the first-use tables
    included, and leaves room for a slow disk"""
    exe = compile_driver(str(tmp_path_factory.mktemp("nr_exe") / "ntt_rows_driver"))
    d = str(tmp_path_factory.mktemp("nr_cases"))
    os.makedirs(os.path.join(d, "in"))
    os.makedirs(os.path.join(d, "out"))
    with open(os.path.join(d, "g.bin"), "wb") as f:
        f.write(orc.ints_to_mont([pyref.FR_GEN])[0].tobytes())
    with open(os.path.join(d, "cases.txt"), "w") as f:
        for s in SHAPES:
            f.write("%s %d %d %d %d\n" % (name(s), s[0], s[1], s[2], len(COLUMNS)))
    for log_n in sorted({s[0] for s in SHAPES}):
        with open(os.path.join(d, "in", "%d.bin" % log_n), "wb") as f:
            f.write(np.ascontiguousarray(columns(log_n)).tobytes())
    t0 = time.time()
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=60)
    print("ntt_rows_driver: ran in %.1f s: %s" % (time.time() - t0, r.stdout.strip()[-200:]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d cases run" % len(SHAPES) in r.stdout

    def read(shape, which, words):
        """the array of `words` field elements and whether the guard behind it is intact"""
        raw = np.fromfile(os.path.join(d, "out", "%s.%s.bin" % (name(shape), which)), dtype=np.uint8)
        assert raw.size == words * 32 + GUARD, (shape, which, raw.size)
        return raw[:words * 32].view(np.uint64).reshape(words, 4), bool((raw[words * 32:] == 0xA5).all())
    yield read
    shutil.rmtree(d, ignore_errors=True)


def coset_rows(coeffs, log_n, lef, rows, g):
    """the oracle's extension of every column, in the layout of ctx.hpp: column c, coset k1 at (c * rows + k1) * n"""
    n, E = 1 << log_n, 1 << lef
    nat = orc.coset_ntt_cols(coeffs, log_n + lef, g)   # orc_coset_ntt per column: nat[c][k1 + E k2] = f_c(g w_ext^(k1 + E k2))
    return nat.reshape(len(coeffs), n, E, 4).transpose(0, 2, 1, 3)[:, :rows].reshape(len(coeffs) * rows * n, 4)


@pytest.mark.parametrize("shape", SHAPES, ids=name)
def test_coset_rows_and_extend_lagrange(outputs, shape):
    """every output word of both calls against the oracle; the words behind each buffer and the input left as they were"""
    log_n, lef, rows = shape
    n = 1 << log_n
    a = columns(log_n)
    cols = len(a)
    g = orc.ints_to_mont([pyref.FR_GEN])[0]

    coeffs = orc.ntt(a, log_n, True)
    want = coset_rows(np.concatenate([a, coeffs]), log_n, lef, rows, g)   # one oracle call for both inputs: it runs the columns in parallel

    got, guard = outputs(shape, "rows", cols * rows * n)
    assert guard, "zk_coset_ntt_rows wrote past its %d rows per column" % rows
    assert np.array_equal(got, want[:cols * rows * n]), "zk_coset_ntt_rows"

    got, guard = outputs(shape, "ext", cols * rows * n)
    assert guard, "zk_extend_lagrange wrote past its %d rows per column" % rows
    assert np.array_equal(got, want[cols * rows * n:]), "zk_extend_lagrange: out"
    tmp, guard = outputs(shape, "tmp", cols * n)
    assert guard, "zk_extend_lagrange wrote past tmp"
    if log_n != 13:   # at 2^13 tmp is the coefficients times n: only `out` is specified there
        assert np.array_equal(tmp, coeffs.reshape(cols * n, 4)), "zk_extend_lagrange: tmp"
    src, guard = outputs(shape, "src", cols * n)
    assert guard and np.array_equal(src, a.reshape(cols * n, 4)), "the input columns changed"
