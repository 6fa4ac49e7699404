"""The prover's own NTT path, which the C API does not reach: zk_coset_ntt_rows (the first `rows` cosets of an extension, fewer than
2^lef of them, written densely) and zk_extend_lagrange (Lagrange columns -> coefficients -> coset rows), bit for bit against the CPU
oracle, at tile sizes below 2^13 and at the row lengths that take a table of coset powers -- whole proofs (k = 13, 14, 16, 19) never
run those -- up to 2^20, where an LDS pass reads the table and a register pass follows it.  And the schedule without LDS passes
(ZKFHE_NTT_LDS_PASS=0: register passes of three stages), which the library chooses once per process: plain transforms of 2^17, 2^18
and 2^20 points, the row calls at 2^17 and 2^19, and enough columns of 2^17 to send k_dif_fused<3> through its grid loop twice.
tests/native/ntt_rows_driver.hip makes the calls: compiled once with the library's flags, linked against the built library, run
twice as a child process, the second time with the variable in the child's environment only; the tests only compare arrays.  The
oracle knows nothing of the variable.  The shapes are those of tests/ntt_schedules.py, which tests/test_ntt_schedules_host.py holds
against the plans.

Measured on an MI355X box (256 CUs, 16 host cores), the slowest three tests: the rows of 2^20 x 3 cosets 3.3 s and of 2^19 x 5
cosets 2.9 s -- each nearly all of it the oracle's four extended columns of 2^22 points, 5.8 s apiece on one core where this was
written, side by side there -- and the plain transforms of 2^20 without LDS passes 2.3 s (the oracle: 1.5 s a column and direction).
The driver's two runs take 1.1 s and 1.0 s, the compile before them 0.8 s.
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref
from tests import ntt_schedules as ns
from tests.test_gpu_ntt_edges import COSET_PATTERNS, batch
from tests.test_product_bounds_host import LARGE_SIZE_PATTERNS, R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ntt_rows_driver.hip")
GUARD = 4096   # bytes of 0xA5 behind every output buffer

SHAPES = ns.ROW_SHAPES   # (log_n, lef, rows)
COLUMNS = COSET_PATTERNS + ("random",)   # the structured columns of the coset tests and one random column
TWO_COLUMNS = ("const r-1", "random")    # from 2^18 on: the output files of a shape stay below 0.3 GB each
FWD_TO, FWD_IN, INV_TO, INV_IN = 1, 2, 4, 8   # the driver's CALLS
CALLS = {"fwd_to": (FWD_TO, False), "fwd_in": (FWD_IN, False), "inv_to": (INV_TO, True), "inv_in": (INV_IN, True)}


def name(shape):
    return "n%d_e%d_r%d" % shape


_columns = {}


def columns(log_n):
    """(4, n, 4), from 2^18 on (2, n, 4): the same columns serve as coefficients (zk_coset_ntt_rows), as Lagrange values
    (zk_extend_lagrange) and as the input of the plain transforms"""
    if log_n not in _columns:
        only = COLUMNS if log_n < ns.TWO_COLUMN_ROWS else TWO_COLUMNS
        pats, a = batch(log_n, only=only)
        assert sorted(p[0] for p in pats) == sorted(only)
        a.setflags(write=False)
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


_gave_up = []   # a driver run that failed: nothing more is launched from this module


def run_driver(exe, d, cases, inputs, env=None, lds="on", limit=120):
    """One run of the driver as a child process on the case lines `cases` and the input arrays {file name: array}.  Returns
    read(name, which, words): the array of `words` field elements in out/<name>.<which>.bin and whether the guard behind it is intact."""
    if _gave_up:
        pytest.fail("not run: %s" % _gave_up[0])
    os.makedirs(os.path.join(d, "in"))
    os.makedirs(os.path.join(d, "out"))
    with open(os.path.join(d, "g.bin"), "wb") as f:
        f.write(orc.ints_to_mont([pyref.FR_GEN])[0].tobytes())
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("".join(line + "\n" for line in cases))
    for fname, a in inputs.items():
        with open(os.path.join(d, "in", fname), "wb") as f:
            f.write(np.ascontiguousarray(a).tobytes())
    t0 = time.time()
    try:
        r = subprocess.run([exe, d], capture_output=True, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        _gave_up.append("an earlier run of ntt_rows_driver did not end within %d s" % limit)
        raise
    print("ntt_rows_driver: ran in %.1f s: %s" % (time.time() - t0, r.stdout.strip()[-200:]))
    if r.returncode != 0:
        _gave_up.append("an earlier run of ntt_rows_driver ended with status %d" % r.returncode)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d cases run" % len(cases) in r.stdout and "LDS passes: %s\n" % lds in r.stdout

    def read(case, which, words):
        raw = np.fromfile(os.path.join(d, "out", "%s.%s.bin" % (case, which)), dtype=np.uint8)
        assert raw.size == words * 32 + GUARD, (case, which, raw.size)
        return raw[:words * 32].view(np.uint64).reshape(words, 4), bool((raw[words * 32:] == 0xA5).all())
    return read


def rows_case(shape):
    return "rows %s %d %d %d %d %d.bin" % (name(shape), shape[0], shape[1], shape[2], len(columns(shape[0])), shape[0])


def plain_case(log_n, calls=FWD_TO | FWD_IN | INV_TO | INV_IN):
    return "plain p%d %d %d %d.bin %d" % (log_n, log_n, len(columns(log_n)), log_n, calls)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_driver(str(tmp_path_factory.mktemp("nr_exe") / "ntt_rows_driver"))


@pytest.fixture(scope="module")
def outputs(exe, tmp_path_factory):
    """the driver's first run, as the library is by default: 24 row calls on rows of at most 2^20 points, the plain transforms of 2^16
    and 2^19, and 1.7 GB of output files.  The limit covers that step alone, context creation and the first-use tables included, and
    leaves room for a slow disk"""
    d = str(tmp_path_factory.mktemp("nr_cases"))
    sizes = sorted({s[0] for s in SHAPES} | set(ns.PLAIN_CASES))
    env = {k: v for k, v in os.environ.items() if k != "ZKFHE_NTT_LDS_PASS"}
    read = run_driver(exe, d, [rows_case(s) for s in SHAPES] + [plain_case(log_n) for log_n in ns.PLAIN_CASES], {"%d.bin" % log_n: columns(log_n) for log_n in sizes}, env=env)
    yield read
    shutil.rmtree(d, ignore_errors=True)


def loop_columns(num_cu):
    """(the eight distinct columns of 2^17, which of them each of the num_cu // 4 + 3 columns is).  k_dif_fused<3> is launched with
    at most num_cu * 16 workgroups of 256 threads, each thread eight points of a column: a thread's second trip lies num_cu // 4
    columns further on, in a column that holds other values."""
    log_n = ns.FALLBACK_LOOP[0]
    n = 1 << log_n
    quarter = num_cu // 4
    C = quarter + 3
    assert C * (n >> 3) > num_cu * 16 * 256, "every butterfly of k_dif_fused<3> has a thread of its own: no second trip on this device"
    pats, a6 = batch(log_n, only=LARGE_SIZE_PATTERNS)
    assert len(pats) == 6
    eight = np.concatenate([a6, ns.random_words(log_n, n)[None], ns.random_words(100 + log_n, n)[None]])
    assert len({eight[i].tobytes() for i in range(8)}) == 8
    idx = []
    for c in range(C):
        idx.append(c % 8 if c < quarter else (idx[c - quarter] + 1) % 8)
    assert all(idx[quarter + j] != idx[j] for j in range(C - quarter))
    return eight, idx


@pytest.fixture(scope="module")
def fallback_outputs(exe, outputs, tmp_path_factory):
    """the driver's second run, with ZKFHE_NTT_LDS_PASS=0 in the child's environment and nowhere else.  It follows the first (the
    fixture asks for it), so a fault there keeps this one from starting.  Yields (read, eight, idx): the loop case's columns."""
    if _gave_up:
        pytest.fail("not run: %s" % _gave_up[0])
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    num_cu = c.device_info()["num_cu"]
    c.close()
    eight, idx = loop_columns(num_cu)
    log_n = ns.FALLBACK_LOOP[0]
    d = str(tmp_path_factory.mktemp("nr_fallback"))
    cases = [plain_case(log_n) for log_n in ns.FALLBACK_PLAIN] + [rows_case(s) for s in ns.FALLBACK_ROWS]
    cases.append("plain loop %d %d loop.bin %d" % (log_n, len(idx), FWD_TO | INV_IN))
    inputs = {"%d.bin" % log_n: columns(log_n) for log_n in sorted(set(ns.FALLBACK_PLAIN) | {s[0] for s in ns.FALLBACK_ROWS})}
    inputs["loop.bin"] = eight[idx]
    read = run_driver(exe, d, cases, inputs, env=dict(os.environ, ZKFHE_NTT_LDS_PASS="0"), lds="off")
    del inputs
    yield read, eight, idx
    shutil.rmtree(d, ignore_errors=True)


def coset_rows(coeffs, log_n, lef, rows, g):
    """the oracle's extension of every column, in the layout of ctx.hpp: column c, coset k1 at (c * rows + k1) * n"""
    n, E = 1 << log_n, 1 << lef
    nat = orc.coset_ntt_cols(coeffs, log_n + lef, g)   # orc_coset_ntt per column: nat[c][k1 + E k2] = f_c(g w_ext^(k1 + E k2))
    return nat.reshape(len(coeffs), n, E, 4).transpose(0, 2, 1, 3)[:, :rows].reshape(len(coeffs) * rows * n, 4)


_want = {}


def expected(shape):
    """(the coefficients of the columns, the oracle's rows of both calls), once per shape: the two runs of the driver share them"""
    if shape not in _want:
        log_n, lef, rows = shape
        a = columns(log_n)
        g = orc.ints_to_mont([pyref.FR_GEN])[0]
        coeffs = orc.ntt(a, log_n, True)
        want = coset_rows(np.concatenate([a, coeffs]), log_n, lef, rows, g)   # one oracle call for both inputs: it runs the columns in parallel
        if shape not in ns.FALLBACK_ROWS:
            return coeffs, want
        _want[shape] = (coeffs, want)
    return _want[shape]


def check_rows(read, shape):
    """every output word of both calls against the oracle; the words behind each buffer and the input left as they were"""
    log_n, lef, rows = shape
    n = 1 << log_n
    a = columns(log_n)
    cols = len(a)
    coeffs, want = expected(shape)

    got, guard = read(name(shape), "rows", cols * rows * n)
    assert guard, "zk_coset_ntt_rows wrote past its %d rows per column" % rows
    assert np.array_equal(got, want[:cols * rows * n]), "zk_coset_ntt_rows"

    got, guard = read(name(shape), "ext", cols * rows * n)
    assert guard, "zk_extend_lagrange wrote past its %d rows per column" % rows
    assert np.array_equal(got, want[cols * rows * n:]), "zk_extend_lagrange: out"
    tmp, guard = read(name(shape), "tmp", cols * n)
    assert guard, "zk_extend_lagrange wrote past tmp"
    if log_n != 13:   # at 2^13 tmp is the coefficients times n: only `out` is specified there
        assert np.array_equal(tmp, coeffs.reshape(cols * n, 4)), "zk_extend_lagrange: tmp"
    src, guard = read(name(shape), "src", cols * n)
    assert guard and np.array_equal(src, a.reshape(cols * n, 4)), "the input columns changed"


def check_plain(read, case, a, calls, want):
    """the files of one plain case: a (cols, n, 4) went in, want(inverse)[c] is the transform of column c"""
    cols, n = a.shape[0], a.shape[1]
    for which, (bit, inverse) in CALLS.items():
        if calls & bit:
            got, guard = read(case, which, cols * n)
            assert guard, "%s wrote past its %d columns" % (which, cols)
            w = want(inverse)
            bad = [c for c in range(cols) if not np.array_equal(got[c * n:(c + 1) * n], w(c))]
            assert not bad, "%s: columns %s" % (which, bad[:20])
    src, guard = read(case, "src", cols * n)
    assert guard and np.array_equal(src, a.reshape(cols * n, 4)), "the input columns changed"


def oracle_of(a, log_n):
    def want(inverse):
        t = orc.ntt(a, log_n, inverse)
        if not inverse:   # the constant r - 1 in closed form: n (r - 1) at 0, exact zeros elsewhere
            consts = [c for c in range(len(a)) if not (a[c] != a[c][0]).any()]
            assert consts and all(orc.arr_to_ints(t[c][:1]) == [orc.arr_to_ints(a[c][:1])[0] * len(a[c]) % R] and not t[c][1:].any() for c in consts)
        return lambda c: t[c]
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=name)
def test_coset_rows_and_extend_lagrange(outputs, shape):
    check_rows(outputs, shape)


@pytest.mark.parametrize("log_n", list(ns.PLAIN_CASES))
def test_plain_transforms(outputs, log_n):
    """the driver's plain calls as the library is by default, at the four-step sizes: in place and out of place, both directions"""
    a = columns(log_n)
    check_plain(outputs, "p%d" % log_n, a, 15, oracle_of(a, log_n))


@pytest.mark.parametrize("log_n", list(ns.FALLBACK_PLAIN))
def test_fallback_plain_transforms(fallback_outputs, log_n):
    """without LDS passes: 2^17 as k_dif_fused<3> and k_dif_stage, 2^18 as k_dif_fused<3> and k_dif_fused<2>, 2^20 as three passes, each
    chain in place (on the data, the tiles into scratch, one copy back) and out of place (source -> scratch -> destination)"""
    a = columns(log_n)
    check_plain(fallback_outputs[0], "p%d" % log_n, a, 15, oracle_of(a, log_n))


@pytest.mark.parametrize("shape", list(ns.FALLBACK_ROWS), ids=name)
def test_fallback_coset_rows_and_extend_lagrange(fallback_outputs, shape):
    """without LDS passes the table of coset powers is read by k_dif_fused<3>: 2^17 with k_dif_stage behind it, 2^19 x 5 rows with a
    second k_dif_fused<3>"""
    check_rows(fallback_outputs[0], shape)


def test_fallback_second_trip_of_the_grid_loop(fallback_outputs):
    """num_cu // 4 + 3 columns of 2^17 drawn from eight, forward out of place and inverse in place: the oracle transforms the eight"""
    read, eight, idx = fallback_outputs
    log_n = ns.FALLBACK_LOOP[0]
    want = {inverse: orc.ntt(eight, log_n, inverse) for inverse in (False, True)}
    check_plain(read, "loop", eight[idx], FWD_TO | INV_IN, lambda inverse: lambda c: want[inverse][idx[c]])
