"""Every pass schedule of the long-row NTT (ntt_long_rows in csrc/ntt.hip, planned by csrc/ntt_plan.hpp) that the C ABI reaches and no
other test runs, bit for bit against a reference on the host:

  rows of 2^21 .. 2^24 points   an LDS pass of six stages (k_dif_lds<3>) with k_dif_fused<2>, k_dif_fused<3>, k_dif_lds<1> or
                                k_dif_lds<2> behind it, in place and out of place;
  2^18                          k_dif_lds<2> on the structured columns of tests/test_gpu_ntt_edges.py, which stops at 2^17;
  many columns                  of 2^17, 2^14, 2^15, 2^18 and 2^21 points: more tiles / threads than the launch of k_dif_lds<1>,
                                k_dif_stage, k_dif_fused<2>, k_dif_lds<2> and k_dif_lds<3> is capped at, so that every workgroup takes
                                a second trip through its grid loop -- in k_dif_lds the trip whose first barrier keeps the next tile
                                out of LDS that another wave still reads;
  zkfhe_coset_ntt_batch         at 2^17 x 4, 2^18 x 2, 2^19 x 8 and 2^20 x 2: the table of coset powers read by each LDS pass
                                (2^19 x 8 is the one shape that brings k_dif_lds<3> to the table), and the inverse's row transforms
                                into scratch slot 2 with k_ext_combine behind them.

The sizes come from tests/ntt_schedules.py, which tests/test_ntt_schedules_host.py holds against the plans.  The prover's own row calls
and the schedules without LDS passes are in tests/test_gpu_ntt_rows.py.

The reference is the CPU oracle up to 2^21 points.  Beyond that one oracle column costs seconds (5.8 s at 2^22 on the machine this was
written on), and the rows are checked by the identity of tests/ntt_schedules.py in a random point instead: 0.33 s at 2^22, and a wrong
word survives with probability at most n / r < 2^-229.  2^25 and 2^26 are not run: a host-side reference costs tens of seconds there,
and their passes (six, four and three stages) are the ones that 2^21 .. 2^24 run.

Measured on an MI355X box (256 CUs, 16 host cores), the slowest three tests: 2^24 2.2 s (two identities of 2^24 words, the rest
copies of 0.5 GB), the eleven columns of 2^21 1.7 s a direction (the oracle's two columns, 3 s apiece on one core where this was
written, side by side there; the test of 2^21 after it reuses them), 2^20 x 2 cosets 1.3 s a direction (one oracle column of 2^21).
The whole module: 25 tests in 15 s.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref
from tests import ntt_schedules as ns
from tests.test_gpu_ntt_edges import batch, check_closed_forms, run_to
from tests.test_product_bounds_host import LARGE_SIZE_PATTERNS, R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


_patterns = {}


def patterns(log_n):
    """the six structured columns of the large sizes, built once per size and never written to"""
    if log_n not in _patterns:
        pats, a = batch(log_n, only=LARGE_SIZE_PATTERNS)
        assert sorted(p[0] for p in pats) == sorted(LARGE_SIZE_PATTERNS)
        a.setflags(write=False)
        _patterns[log_n] = (pats, a)
    return _patterns[log_n]


# ---- b. 2^18: k_dif_lds<2> alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log_n", sorted(ns.STRUCTURED_SIZES))
def test_structured_columns(ctx, log_n, inverse):
    """the constant r - 1, the alternating (w, r - w), the single r - 1, the spike-producing geometric column, the inverse image of
    "all r - 1" and the random control: against the oracle and, where there is one, the closed form"""
    pats, a = patterns(log_n)
    assert len(pats) == 6
    which = 3 if inverse else 2
    want = orc.ntt(a, log_n, inverse)
    check_closed_forms(pats, want, which, log_n)
    for route, got in (("in place", ctx.ntt(a, log_n, inverse)), ("out of place", run_to(ctx, a, log_n, inverse))):
        bad = [pats[c][0] for c in range(6) if not np.array_equal(got[c], want[c])]
        assert not bad, "%s: %s" % (route, bad)
        check_closed_forms(pats, got, which, log_n)


# ---- c. second trips of the grid loops ---------------------------------------------------------------------------------------------
_two = {}


def two_columns(log_n, inverse=None):
    """the random control and the constant r - 1 (inverse is None), or the oracle's transform of them: once per size and direction"""
    if (log_n, None) not in _two:
        n = 1 << log_n
        _two[log_n, None] = np.stack([ns.random_words(log_n, n), ns.const_words(R - 1, n)])
    if (log_n, inverse) not in _two:
        n = 1 << log_n
        want = orc.ntt(_two[log_n, None], log_n, inverse)
        # the constant's transform in closed form: n (r - 1), or r - 1 after the inverse, at 0 and exact zeros elsewhere
        assert orc.arr_to_ints(want[1][:1]) == [(R - 1) if inverse else n * (R - 1) % R] and not want[1][1:].any()
        _two[log_n, inverse] = want
    for a in _two.values():
        a.setflags(write=False)
    return _two[log_n, inverse]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log_n", list(ns.LOOP_SIZES))
def test_second_trip_of_the_grid_loop(ctx, log_n, inverse):
    """More columns than the launch of the first pass covers.  The LDS pass is capped at num_cu * 64 workgroups of one 1024-point tile
    each, a register pass of S stages at num_cu * 16 workgroups of 256 threads with 2^S points each; a whole number `shift` of
    columns fills that, and with shift + 3 columns a workgroup's second tile (a thread's second butterfly) lies `shift` columns
    further on -- num_cu // 2 + 3 columns of 2^17 (k_dif_lds<1>), 2^14 (k_dif_stage) and 2^15 (k_dif_fused<2>), num_cu // 4 + 3 of
    2^18 (k_dif_lds<2>), num_cu // 32 + 3 of 2^21 (k_dif_lds<3>, and many trips of k_dif_fused<2> behind it).  In k_dif_lds that is the
    trip whose first barrier keeps the next tile out of LDS that another wave may still be reading.  The columns are drawn from
    eight (the six structured ones and two random; at 2^21, where the oracle takes seconds per column, the random control and the
    constant r - 1) so that column shift + j never holds what column j holds; the oracle transforms the distinct ones only.  They
    go to the device one by one and come back one by one: no host array holds them all."""
    n = 1 << log_n
    num_cu = ctx.device_info()["num_cu"]
    first = ns.LOOP_SIZES[log_n].split()[0]
    if first.endswith("L"):
        per_column, cap = n // 1024, num_cu * 64          # tiles, workgroups
    else:
        per_column, cap = n >> int(first), num_cu * 16 * 256   # butterflies, threads
    assert cap % per_column == 0, "the second trip does not start at a column's first point on this device"
    shift = cap // per_column
    C = shift + 3
    assert C == {17: num_cu // 2, 14: num_cu // 2, 15: num_cu // 2, 18: num_cu // 4, 21: num_cu // 32}[log_n] + 3
    assert C * per_column > cap, "everything has a workgroup (a thread) of its own: no second trip on this device"
    if log_n < 20:
        pats, a6 = patterns(log_n)
        distinct = np.concatenate([a6, ns.random_words(log_n, n)[None], ns.random_words(100 + log_n, n)[None]])
        want = orc.ntt(distinct, log_n, inverse)
    else:
        distinct, want = two_columns(log_n), two_columns(log_n, inverse)
    k = len(distinct)
    assert len({distinct[i].tobytes() for i in range(k)}) == k
    idx = []
    for c in range(C):
        idx.append(c % k if c < shift else (idx[c - shift] + 1) % k)
    assert all(idx[shift + j] != idx[j] for j in range(C - shift)) and set(idx) == set(range(k))

    def mismatches(d, ref):
        return [(c, idx[c]) for c in range(C) if not np.array_equal(d.download(shape=(n, 4), byte_offset=c * n * 32, nbytes=n * 32), ref[idx[c]])]

    src, dst = ctx.alloc(C * n * 32), ctx.alloc(C * n * 32)
    for c in range(C):
        src.upload(distinct[idx[c]], c * n * 32)
    ctx.ntt_to_dev(src, dst, C, log_n, inverse=inverse)
    bad = mismatches(dst, want)
    assert not bad, "out of place: (column, which of the distinct ones) %s" % bad[:20]
    assert not mismatches(src, distinct), "ntt_to_dev wrote to its source"
    dst.free()
    ctx.ntt_dev(src, C, log_n, inverse)
    bad = mismatches(src, want)
    assert not bad, "in place: (column, which of the distinct ones) %s" % bad[:20]
    src.free()


# ---- d. the coset extension through the public call ------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log_n,lef", list(ns.COSET_CALLS))
def test_coset_call(ctx, log_n, lef, inverse):
    """One random column through ctx.coset_ntt, in the layout of test_coset_ntt: row k1 of the extension holds f(g w_ext^(k1 + E k2)).
    2^17 x 4, 2^18 x 2 and 2^20 x 2 against the oracle's coset transform (one call per case: at most 2^21 values); 2^19 x 8 has 2^22
    values, which the oracle takes 6 s for, so both its directions are held to the identity on the coset instead (0.4 s) -- forward
    f's coefficients in and its values out, inverse values in and coefficients out, the same identity between them."""
    n, E, N = 1 << log_n, 1 << lef, 1 << (log_n + lef)
    g = orc.ints_to_mont([pyref.FR_GEN])[0]
    w_ext, rho = pyref.root_of_unity(log_n + lef), ns.point(log_n * 10 + lef)
    by_identity = log_n + lef > 21

    def natural(rows):   # nat[k1 + E k2] <- rows[k1][k2]
        return rows.reshape(E, n, 4).transpose(1, 0, 2).reshape(N, 4)

    def coset_major(nat):
        return nat.reshape(n, E, 4).transpose(1, 0, 2).reshape(N, 4)

    if not inverse:
        a = ns.random_words(log_n * 10 + lef, n)
        got = ctx.coset_ntt(a[None], log_n, lef, g)[0]
        if by_identity:
            assert ns.transform_identity_holds(a, natural(got), w_ext, 1, rho, g=pyref.FR_GEN)
        else:
            assert np.array_equal(got, coset_major(orc.coset_ntt(a, log_n + lef, g)))
    elif by_identity:
        nat = ns.random_words(log_n * 10 + lef + 1, N)   # any N values are those of one polynomial of degree < N
        back = ctx.coset_ntt(coset_major(nat)[None], log_n, lef, g, inverse=True)[0]
        assert ns.transform_identity_holds(back, nat, w_ext, 1, rho, g=pyref.FR_GEN)
    else:
        coeffs = ns.random_words(log_n * 10 + lef + 1, N)
        ext = coset_major(orc.coset_ntt(coeffs, log_n + lef, g))
        assert np.array_equal(ctx.coset_ntt(ext[None], log_n, lef, g, inverse=True)[0], coeffs)


# ---- a. 2^21 .. 2^24 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_rows_of_2_21_against_the_oracle(ctx, inverse):
    """the random control and the constant r - 1, in place and out of place, and back again"""
    log_n = 21
    a, want = two_columns(log_n), two_columns(log_n, inverse)   # shared with the loop test of this size
    got = ctx.ntt(a, log_n, inverse)
    assert np.array_equal(got, want), "in place"
    assert np.array_equal(run_to(ctx, a, log_n, inverse), want), "out of place"
    assert np.array_equal(ctx.ntt(got, log_n, not inverse), a), "the round trip"


@pytest.mark.parametrize("log_n", [s for s in sorted(ns.LARGE_SIZES) if s > 21])
def test_large_rows(ctx, log_n):
    """One random column.  Forward in place, held to the identity in a random point; from that result the inverse out of place, which
    must give the column back and leave its source as it was; and the inverse of the column itself out of place, held to the
    identity of the inverse."""
    n = 1 << log_n
    x = ns.random_words(log_n, n)
    rho = ns.point(log_n)
    d, back = ctx.to_device(x), ctx.alloc(n * 32)
    ctx.ntt_dev(d, 1, log_n, False)
    X = d.download(shape=(n, 4))
    assert ns.ntt_identity_holds(x, X, log_n, False, rho), "forward, in place"
    ctx.ntt_to_dev(d, back, 1, log_n, inverse=True)
    assert np.array_equal(back.download(shape=(n, 4)), x), "inverse(forward(x)) is not x"
    assert np.array_equal(d.download(shape=(n, 4)), X), "ntt_to_dev wrote to its source"
    del X
    d.upload(x)
    ctx.ntt_to_dev(d, back, 1, log_n, inverse=True)
    Y = back.download(shape=(n, 4))
    assert np.array_equal(d.download(shape=(n, 4)), x), "ntt_to_dev wrote to its source"
    assert ns.ntt_identity_holds(x, Y, log_n, True, rho), "inverse, out of place"
    ctx.ntt_dev(back, 1, log_n, False)
    assert np.array_equal(back.download(shape=(n, 4)), x), "forward(inverse(x)) is not x"
    d.free(), back.free()
