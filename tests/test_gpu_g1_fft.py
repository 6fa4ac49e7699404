"""zkfhe_g1_fft on the GPU against the CPU oracle: the naive DFT over G1 as oracle MSMs, byte for byte (canonical affine Montgomery
limbs: no tolerance anywhere).

Sizes: every log_n from 1 to 13 and 16, both directions.  The launcher switches between kernel structures once: up to log_n = 6 every
stage runs k_g1_fft_window, from log_n = 7 = G1FFT_FIRST_SHARED_LOG (csrc/g1_fft_plan.hpp; tests/test_g1_fft_host.py pins it) the
stages with at least 64 blocks run k_g1_fft_shared -- SWITCH names the two sides.
Up to 256 points every output is checked (n oracle MSM columns); above, outputs 0, 1, n/2 + 1 and n - 1."""
import numpy as np
import pytest

from oracle import binding as orc
from oracle import halo2_ref as H
from oracle import pyref

pytestmark = pytest.mark.gpu

SWITCH = (6, 7)          # the last size of window stages only | the first with shared-twiddle stages
SIZES = list(range(1, 14)) + [16]
DEGENERATE_SIZES = (3, 6, 7)   # 7: the smallest size that launches both structures


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def M(v):
    return orc.ints_to_mont([v % pyref.R])[0]


GEN = None


def gen():
    global GEN
    if GEN is None:
        GEN = orc.points_to_arr([pyref.G1_GEN])[0]
    return GEN


def mul_gen(scalars_mont):
    s = np.ascontiguousarray(scalars_mont, dtype=np.uint64).reshape(-1, 4)
    return orc.g1_mul(np.repeat(gen()[None], s.shape[0], axis=0), s)


@pytest.fixture(scope="module")
def random_points():
    """2^16 random multiples of the generator, made once; a test of 2^log_n points takes the first 2^log_n"""
    rng = np.random.default_rng(1607)
    k = orc.ints_to_mont([int.from_bytes(rng.bytes(32), "little") % pyref.R for _ in range(1 << 16)])
    pts = mul_gen(k)
    pts.setflags(write=False)
    return pts


def rows_of(n):
    return list(range(n)) if n <= 256 else [0, 1, n // 2 + 1, n - 1]


def naive(points, log_n, inverse, rows):
    """out[i] = (n^-1) sum_j w^(+-ij) P_j for i in rows: one oracle MSM, a column per output"""
    n = 1 << log_n
    w = pyref.root_of_unity(log_n)
    if inverse:
        w = pow(w, -1, pyref.R)
    scale = pow(n, -1, pyref.R) if inverse else 1
    tw = [scale] * n
    for j in range(1, n):
        tw[j] = tw[j - 1] * w % pyref.R
    scal = orc.ints_to_mont([tw[(i * j) & (n - 1)] for i in rows for j in range(n)]).reshape(len(rows), n, 4)
    return orc.msm(scal, points)


def check(ctx, points, log_n, inverse):
    n = 1 << log_n
    rows = rows_of(n)
    got = ctx.g1_fft(points, inverse=inverse)
    assert got.shape == (n, 8)
    want = naive(points, log_n, inverse, rows)
    assert np.array_equal(got[rows], want), "log_n %d inverse %s" % (log_n, inverse)
    return got


def test_switch_sizes_are_covered():
    assert SWITCH[0] + 1 == SWITCH[1] and all(s in SIZES for s in SWITCH)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", SIZES)
def test_random_points(ctx, random_points, log_n, inverse):
    check(ctx, np.array(random_points[:1 << log_n]), log_n, inverse)


@pytest.mark.parametrize("log_n", DEGENERATE_SIZES)
def test_all_generator_inverse(ctx, log_n):
    """every butterfly doubles or cancels: G at index 0, the identity elsewhere"""
    n = 1 << log_n
    got = check(ctx, np.repeat(gen()[None], n, axis=0), log_n, True)
    assert np.array_equal(got[0], gen()) and not got[1:].any()


@pytest.mark.parametrize("log_n", DEGENERATE_SIZES)
def test_powers_of_omega_inverse(ctx, log_n):
    """P_j = w^j G: G at index 1, the identity elsewhere"""
    n = 1 << log_n
    pts = mul_gen(orc.fr_powers(M(1), M(pyref.root_of_unity(log_n)), n))
    got = check(ctx, pts, log_n, True)
    assert np.array_equal(got[1], gen()) and not got[0].any() and not got[2:].any()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", DEGENERATE_SIZES)
def test_all_identity(ctx, log_n, inverse):
    assert not ctx.g1_fft(np.zeros((1 << log_n, 8), dtype=np.uint64), inverse=inverse).any()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", DEGENERATE_SIZES)
def test_identity_at_odd_indices(ctx, random_points, log_n, inverse):
    pts = np.array(random_points[:1 << log_n])
    pts[1::2] = 0
    check(ctx, pts, log_n, inverse)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", DEGENERATE_SIZES)
def test_lone_point(ctx, random_points, log_n, inverse):
    pts = np.zeros((1 << log_n, 8), dtype=np.uint64)
    pts[(1 << log_n) - 3] = random_points[5]
    check(ctx, pts, log_n, inverse)


def test_round_trip(ctx, random_points):
    pts = np.array(random_points[:1 << 13])
    assert np.array_equal(ctx.g1_fft(ctx.g1_fft(pts), inverse=True), pts)


@pytest.mark.parametrize("k", [3, 9, 13])
def test_lagrange_basis_of_the_oracle_srs(ctx, k):
    """g_to_lagrange: the inverse transform of the oracle's monomial powers is its closed-form Lagrange basis L_i(s) G"""
    srs = H.make_srs(k)
    assert np.array_equal(ctx.g1_fft(srs["g"], inverse=True), srs["g_lagrange"])


def test_refusals(ctx):
    import ctypes
    import zk_fhe_amd as zk
    d = ctx.to_device(np.zeros((2, 8), dtype=np.uint64))
    for log_n in (0, 21, -1):
        assert ctx.lib.zkfhe_g1_fft(ctx.h, ctx._p(d), log_n, 0) == -1
        assert ctx.lib.zkfhe_last_error(ctx.h).decode().startswith("g1_fft:")
    assert ctx.lib.zkfhe_g1_fft(ctx.h, ctypes.c_void_p(), 3, 0) == -1
    d.free()
    with pytest.raises(ValueError):
        ctx.g1_fft(np.zeros((3, 8), dtype=np.uint64))
    assert zk.PROF_G1_FFT == 23


def test_profile_slot_counts_scalar_multiplications(ctx, random_points):
    """slot 23 brackets the butterfly kernels: one launch per stage, 256 B per point and stage, ops = the scalar multiplications
    (none where the twiddle is 1; the n^-1 stage of an inverse call multiplies both operands)"""
    import zk_fhe_amd as zk
    log_n, n = 8, 256
    pts = np.array(random_points[:n])
    for inverse in (False, True):
        ctx.prof_enable(True)
        try:
            ctx.g1_fft(pts, inverse=inverse)
            r = ctx.prof_read(zk.PROF_G1_FFT)
        finally:
            ctx.prof_enable(False)
        mults = sum(n // 2 - (n // 2 >> s) for s in range(log_n))
        if inverse:
            mults += n - (n // 2 - 1)   # the last stage: n instead of n/2 - 1
        assert r["launches"] == log_n and r["algorithmic_bytes"] == 256.0 * n * log_n and r["ops"] == mults and r["total_ms"] > 0
