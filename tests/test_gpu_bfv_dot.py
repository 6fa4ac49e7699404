"""Fused BFV inner products on the GPU (bfv_dot.hip): bit for bit against their definition in zkfhe.h (ref_dot and ref_dot_plain of
tests/test_bfv_dot_host.py), a shared b vector, sums that cross pass boundaries, the CRT bound at its edge with the largest term
count, decryption and noise, the plaintext-weighted sum against bfv_sum of bfv_mul_plain, one rounding and one relinearization per
sum by the profiler's counts, and argument errors.
Run on the MI355X box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

from tests.test_bfv_dot_host import P5, ref_dot, ref_dot_plain
from tests.test_bfv_eval_host import Q29, Q60, Q63, centred, circ, deg, kron_negacyclic, ref_mul, relin_digits
from tests.test_gpu_bfv_encrypt import random_m
from tests.test_gpu_bfv_eval import K13, fresh, random_residues

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def plain_dot(m1, m2, params):
    """sum_i m1_i m2_i mod (x^N + 1, T), centred like the decryption, as residues mod Q (CircuitInput order)"""
    n, q, t = params[0], params[1], params[2]
    x = kron_negacyclic([(centred(deg(u), q), centred(deg(v), q)) for u, v in zip(m1, m2)], n)
    r = [v % t for v in x]
    return circ([v - t if v > t // 2 else v for v in r], q)


def gadget_key(n, q, w):
    """rlk0_i = 2^(i w) as constant polynomials, rlk1_i = 0: sum_i d_i rlk0_i = c^2, so out0 = c^0 + c^2 and out1 = c^1"""
    l = relin_digits(q, w)
    rlk0 = np.zeros((l, n), dtype=np.uint64)
    for i in range(l):
        rlk0[i, n - 1] = 1 << (i * w)
    return rlk0, np.zeros((l, n), dtype=np.uint64)


def monomial_sum(polys, coeffs, shifts, n):
    """sum_i polys[i] * coeffs[i] x^shifts[i] over Z in Z[x]/(x^N + 1) as Python integers: polys of shape (terms, N) in degree order,
    signed below 2^62; |coeffs| <= 2^20.  Signed shifts on int64 halves of 31 bits (each half sum stays below 2^31 2^20 2^9)."""
    lo, hi = polys & ((1 << 31) - 1), polys >> 31   # polys = hi 2^31 + lo, lo in [0, 2^31), hi signed
    acc_lo, acc_hi = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(polys.shape[0]):
        k, v = int(shifts[i]), int(coeffs[i])
        for acc, half in ((acc_lo, lo[i]), (acc_hi, hi[i])):
            acc[k:] += v * half[:n - k]
            acc[:k] -= v * half[n - k:]
    return [int(h) * (1 << 31) + int(l) for h, l in zip(acc_hi, acc_lo)]


def centred_deg(x, q):
    """(terms, N) residues in CircuitInput order -> signed int64 in degree order (Q below 2^62)"""
    x = x[:, ::-1].astype(np.int64)
    return np.where(x > q // 2, x - q, x)


def monomials(rng, terms, n, q):
    coeffs = rng.integers(1, 1 << 20, terms) * rng.choice([-1, 1], terms)
    shifts = rng.integers(0, n, terms)
    out = np.zeros((terms, n), dtype=np.uint64)
    for i in range(terms):
        out[i, n - 1 - shifts[i]] = int(coeffs[i]) % q
    return out, coeffs, shifts


# ---- 1. bit for bit against the definition ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,w,groups,terms", [(1024, Q29, 7, 8, 2, 3), (4096, Q60, 65537, 16, 2, 3), (16384, Q60, 65537, 32, 1, 2)])
def test_dot_bit_exact(ctx, n, q, t, w, groups, terms):
    params = (n, q, t, 19)
    rng = np.random.default_rng(n + w)
    sk, m, c0, c1 = fresh(ctx, params, 2 * terms, bytes([w]) * 32, bytes([w + 1]) * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, bytes([w + 2]) * 32, base_bits=w)
    # group 0: fresh encryptions; the last group: arbitrary residues (a single group: its first term fresh, the rest arbitrary)
    a0, a1, b0, b1 = (random_residues(rng, (groups, terms, n), q) for _ in range(4))
    k = terms if groups > 1 else 1
    a0[0, :k], a1[0, :k], b0[0, :k], b1[0, :k] = c0[:k], c1[:k], c0[terms:terms + k], c1[terms:terms + k]
    out0, out1 = ctx.bfv_dot(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    assert out0.shape == out1.shape == (groups, n) and out0.dtype == np.uint64
    for g in range(groups):
        want0, want1 = ref_dot(params, a0[g], a1[g], b0[g], b1[g], rlk0, rlk1, w)
        assert np.array_equal(out0[g], want0), g
        assert np.array_equal(out1[g], want1), g
    if t == 7:
        assert np.array_equal(ctx.bfv_decrypt(params, sk, out0[:1], out1[:1])[0], plain_dot(m[:terms], m[terms:], params))
    # one term: zkfhe_bfv_mul bit for bit; 2-D inputs give one ciphertext
    g, i = groups - 1, terms - 1
    one0, one1 = ctx.bfv_dot(params, a0[g, i:], a1[g, i:], b0[g, i:], b1[g, i:], rlk0, rlk1, base_bits=w)
    assert one0.shape == one1.shape == (n,)
    mul0, mul1 = ctx.bfv_mul(params, a0[g, i:], a1[g, i:], b0[g, i:], b1[g, i:], rlk0, rlk1, base_bits=w)
    ref0, ref1 = ref_mul(params, a0[g, i], a1[g, i], b0[g, i], b1[g, i], rlk0, rlk1, w)
    assert np.array_equal(one0, mul0[0]) and np.array_equal(one1, mul1[0])
    assert np.array_equal(one0, ref0) and np.array_equal(one1, ref1)


# ---- 2. one b vector for every group --------------------------------------------------------------------------------------------

def test_dot_shared_b(ctx):
    params, w, groups, terms = K13, 8, 3, 2
    n, q = params[0], params[1]
    rng = np.random.default_rng(22)
    sk, _, _ = ctx.bfv_fhe_keypair(params, b"\x71" * 32)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, b"\x72" * 32, base_bits=w)
    a0, a1 = (random_residues(rng, (groups, terms, n), q) for _ in range(2))
    b0, b1 = (random_residues(rng, (terms, n), q) for _ in range(2))
    out0, out1 = ctx.bfv_dot(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    rep0, rep1 = ctx.bfv_dot(params, a0, a1, np.stack([b0] * groups), np.stack([b1] * groups), rlk0, rlk1, base_bits=w)
    assert out0.shape == (groups, n)
    assert np.array_equal(out0, rep0) and np.array_equal(out1, rep1)
    for g in range(groups):
        want0, want1 = ref_dot(params, a0[g], a1[g], b0, b1, rlk0, rlk1, w)
        assert np.array_equal(out0[g], want0) and np.array_equal(out1[g], want1), g


# ---- 3. sums over more than one pass ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("terms", [65, 131])
def test_dot_across_passes(ctx, terms):
    """N = 32768: a pass holds 64 terms, so 65 terms take two passes and 131 three.  Every b_i is a monomial, so that the exact sums
    are signed shifts; with the gadget key out0 = c^0 + c^2 and out1 = c^1.  Every a_i is dense: a dropped, doubled or re-zeroed pass
    changes every coefficient."""
    n, q, t, w = 32768, Q60, 65537, 16
    params = (n, q, t, 19)
    rng = np.random.default_rng(terms)
    a0, a1 = (random_residues(rng, (terms, n), q) for _ in range(2))
    (b0, v0, k0), (b1, v1, k1) = monomials(rng, terms, n, q), monomials(rng, terms, n, q)
    rlk0, rlk1 = gadget_key(n, q, w)
    out0, out1 = ctx.bfv_dot(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    A0, A1 = centred_deg(a0, q), centred_deg(a1, q)
    x0 = monomial_sum(A0, v0, k0, n)
    x1 = [u + v for u, v in zip(monomial_sum(A0, v1, k1, n), monomial_sum(A1, v0, k0, n))]
    x2 = monomial_sum(A1, v1, k1, n)
    rnd = lambda xs: [(2 * t * x + q) // (2 * q) % q for x in xs]  # noqa: E731
    c0h, c1h, c2h = rnd(x0), rnd(x1), rnd(x2)
    assert np.array_equal(out0, circ([u + v for u, v in zip(c0h, c2h)], q))
    assert np.array_equal(out1, circ(c1h, q))


# ---- 4. the CRT bound at its edge -----------------------------------------------------------------------------------------------

def test_dot_crt_bound_at_the_edge(ctx):
    import zk_fhe_amd as zk
    n, q, w = 32768, Q63, 32
    params = (n, q, q - 2, 1)   # T near Q
    t, h = params[2], q // 2
    terms = zk.bfv_dot_max_terms(params)
    # every coefficient +-floor(Q/2) with one sign per polynomial, the same in every term: x_k = terms s v^2 (2k + 2 - N)
    signs = (1, -1, -1, 1)   # a0, a1, b0, b1: x0 and x2 negative, x1 = terms 2 v^2 (2k + 2 - N)
    const = [np.full((terms + 1, n), h if s > 0 else q - h, dtype=np.uint64) for s in signs]
    sa0, sa1, sb0, sb1 = signs
    x0 = [terms * sa0 * sb0 * h * h * (2 * k + 2 - n) for k in range(n)]
    x1 = [terms * (sa0 * sb1 + sa1 * sb0) * h * h * (2 * k + 2 - n) for k in range(n)]
    x2 = [terms * sa1 * sb1 * h * h * (2 * k + 2 - n) for k in range(n)]
    worst = max(abs(x) for x in x1)
    assert worst == terms * 2 * n * h * h and worst <= P5 // 2 < (terms + 1) * 2 * n * h * h
    rlk0, rlk1 = gadget_key(n, q, w)
    out0, out1 = ctx.bfv_dot(params, *[c[:terms] for c in const], rlk0, rlk1, base_bits=w)
    rnd = lambda xs: [(2 * t * x + q) // (2 * q) % q for x in xs]  # noqa: E731
    c0h, c1h, c2h = rnd(x0), rnd(x1), rnd(x2)
    assert np.array_equal(out0, circ([u + v for u, v in zip(c0h, c2h)], q))
    assert np.array_equal(out1, circ(c1h, q))
    with pytest.raises(zk.ZkfheError, match=r"bfv_dot: n_terms %d is above the limit %d\b" % (terms + 1, terms)):
        ctx.bfv_dot(params, *const, rlk0, rlk1, base_bits=w)


# ---- 5. decryption ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,w,terms", [(1024, Q29, 7, 8, 16), (4096, Q60, 7, 16, 5)])
def test_decrypt_after_dot(ctx, n, q, t, w, terms):
    """16 terms at the k = 13 parameters: tests/test_bfv_dot_host.py::test_noise_margin_of_sixteen_terms keeps the host's noise of this
    sum a factor 4 under the decryption bound asserted here."""
    params = (n, q, t, 19)
    rng = np.random.default_rng(q % 1000 + terms)
    sk, m, c0, c1 = fresh(ctx, params, 2 * terms, bytes([w + 6]) * 32, bytes([w + 7]) * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, bytes([w + 8]) * 32, base_bits=w)
    out0, out1 = ctx.bfv_dot(params, c0[:terms], c1[:terms], c0[terms:], c1[terms:], rlk0, rlk1, base_bits=w)
    assert np.array_equal(ctx.bfv_decrypt(params, sk, out0, out1)[0], plain_dot(m[:terms], m[terms:], params))
    noise = ctx.bfv_noise(params, sk, out0, out1)
    assert int(noise[0]) < (q // t) // 2, int(noise[0])


# ---- 6. public weights --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,groups,terms", [(1024, Q29, 7, 2, 5), (4096, Q60, 65537, 1, 3)])
def test_dot_plain(ctx, n, q, t, groups, terms):
    params = (n, q, t, 19)
    rng = np.random.default_rng(n + terms)
    sk, m, c0, c1 = fresh(ctx, params, groups * terms, b"\x81" * 32, b"\x82" * 32, rng)
    c0, c1, m = (x.reshape(groups, terms, n) for x in (c0, c1, m))
    weights = random_m(rng, (groups, terms, n), q, t)
    for shared in (True, False) if groups > 1 else (False,):
        p = weights[0] if shared else weights
        out0, out1 = ctx.bfv_dot_plain(params, c0, c1, p)
        assert out0.shape == out1.shape == (groups, n)
        dec = ctx.bfv_decrypt(params, sk, out0, out1)
        for g in range(groups):
            pg = weights[0] if shared else weights[g]
            s0, s1 = ctx.bfv_sum(params, *ctx.bfv_mul_plain(params, c0[g], c1[g], pg))
            assert np.array_equal(out0[g], s0) and np.array_equal(out1[g], s1), (shared, g)
            want0, want1 = ref_dot_plain(params, c0[g], c1[g], pg)
            assert np.array_equal(out0[g], want0) and np.array_equal(out1[g], want1), (shared, g)
            if t == 7:   # 5 terms of |m p| <= 9 N stay far inside the noise budget
                assert np.array_equal(dec[g], plain_dot(m[g], pg, params)), (shared, g)
    one0, one1 = ctx.bfv_dot_plain(params, c0[0], c1[0], weights[0])   # 2-D inputs give one ciphertext
    want0, want1 = ref_dot_plain(params, c0[0], c1[0], weights[0])
    assert one0.shape == (n,) and np.array_equal(one0, want0) and np.array_equal(one1, want1)


def test_dot_plain_across_passes(ctx):
    n, q, t, terms = 32768, Q60, 65537, 65   # a pass holds 64 terms
    params = (n, q, t, 19)
    rng = np.random.default_rng(65)
    c0, c1 = (random_residues(rng, (terms, n), q) for _ in range(2))
    coeffs = rng.integers(1, t // 2 + 1, terms) * rng.choice([-1, 1], terms)
    shifts = rng.integers(0, n, terms)
    m = np.zeros((terms, n), dtype=np.uint64)
    for i in range(terms):
        m[i, n - 1 - shifts[i]] = int(coeffs[i]) % q
    out0, out1 = ctx.bfv_dot_plain(params, c0, c1, m)
    assert np.array_equal(out0, circ(monomial_sum(centred_deg(c0, q), coeffs, shifts, n), q))
    assert np.array_equal(out1, circ(monomial_sum(centred_deg(c1, q), coeffs, shifts, n), q))


# ---- 7. one rounding and one relinearization per sum ----------------------------------------------------------------------------

def test_one_rounding_per_sum(ctx):
    import zk_fhe_amd as zk
    params, w = K13, 8
    n, q = params[0], params[1]
    rng = np.random.default_rng(7)
    rlk0, rlk1 = (random_residues(rng, (relin_digits(q, w), n), q) for _ in range(2))
    a0, a1, b0, b1 = (random_residues(rng, (8, n), q) for _ in range(4))
    slots = (zk.PROF_BFV_EVAL_EPILOGUE, zk.PROF_BFV_RELIN, zk.PROF_BFV_TENSOR, zk.PROF_BFV_DOT)
    seen = []
    for terms in (8, 1):
        ctx.prof_enable(True)   # resets the counters
        try:
            ctx.bfv_dot(params, a0[:terms], a1[:terms], b0[:terms], b1[:terms], rlk0, rlk1, base_bits=w)
            seen.append([ctx.prof_read(s) for s in slots])
        finally:
            ctx.prof_enable(False)
    for eight, one in list(zip(*seen))[:3]:
        assert eight["launches"] == one["launches"] and eight["algorithmic_bytes"] == one["algorithmic_bytes"]
    assert [r["launches"] for r in seen[0][:3]] == [2, 1, 0]   # EV_ROUND and EV_ADD, one key switch, no k_bfv_tensor
    assert seen[0][3]["launches"] > 0 and seen[1][3]["launches"] > 0
    assert seen[0][3]["algorithmic_bytes"] > seen[1][3]["algorithmic_bytes"] > 0


# ---- 8. argument errors -------------------------------------------------------------------------------------------------------

def test_dot_argument_errors(ctx):
    import zk_fhe_amd as zk
    params, w = K13, 8
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(8)
    sk, m, c0, c1 = fresh(ctx, params, 4, b"\x91" * 32, b"\x92" * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, b"\x93" * 32, base_bits=w)
    a0, a1, b0, b1 = c0[:2], c1[:2], c0[2:], c1[2:]
    g0, g1 = np.stack([a0] * 3), np.stack([a1] * 3)   # three groups

    raw = ctx._call   # the C call itself, past the wrappers' shape checks
    out = [np.empty(n, dtype=np.uint64) for _ in range(2)]
    dot = lambda prm, ng, nt, bg, bb: raw("zkfhe_bfv_dot", prm, ng, nt, a0, a1, bg, b0, b1, rlk0, rlk1, bb, *out)  # noqa: E731
    plain = lambda prm, ng, nt, mg: raw("zkfhe_bfv_dot_plain", prm, ng, nt, a0, a1, mg, m[:2], *out)  # noqa: E731
    # a zero count, a NULL argument, bad parameters
    with pytest.raises(zk.ZkfheError, match="bfv_dot: a NULL argument or a zero count"):
        dot(params, 1, 0, 1, w)
    with pytest.raises(zk.ZkfheError, match="bfv_dot: a NULL argument or a zero count"):
        dot(params, 0, 2, 1, w)
    with pytest.raises(zk.ZkfheError, match="bfv_dot_plain: a NULL argument or a zero count"):
        plain(params, 1, 0, 1)
    f = ctx.lib.zkfhe_bfv_dot_plain
    u64p = ctypes.POINTER(ctypes.c_uint64)
    assert f(ctx.h, ctypes.byref(zk.BfvParamsC(*params)), 1, 2, a0.ctypes.data_as(u64p), a1.ctypes.data_as(u64p), 1, None,
             out[0].ctypes.data_as(u64p), out[1].ctypes.data_as(u64p)) != 0
    assert b"bfv_dot_plain: a NULL argument or a zero count" in ctx.lib.zkfhe_last_error(ctx.h)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        dot((1000, q, t, 19), 1, 2, 1, w)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        plain((n, q, q, 19), 1, 2, 1)   # T >= Q
    # base_bits: before the group counts
    for bad_w in (0, 33):
        with pytest.raises(zk.ZkfheError, match=r"bfv_dot: base_bits must be in \[1, 32\]"):
            dot(params, 1, 2, 2, bad_w)
    # group counts: before the term limit
    edge = (32768, Q63, Q63 - 2, 1)
    limit, limit_plain = zk.bfv_dot_max_terms(edge), zk.bfv_dot_max_terms(edge, plain=True)
    with pytest.raises(zk.ZkfheError, match="bfv_dot: b_groups must be 1 or n_groups"):
        dot(edge, 3, limit + 1, 2, w)
    with pytest.raises(zk.ZkfheError, match="bfv_dot_plain: m_groups must be 1 or n_groups"):
        plain(edge, 3, limit_plain + 1, 2)
    with pytest.raises(zk.ZkfheError, match="bfv_dot: b_groups must be 1 or n_groups"):
        ctx.bfv_dot(params, g0, g1, g0[:2], g1[:2], rlk0, rlk1, base_bits=w)
    with pytest.raises(zk.ZkfheError, match="bfv_dot_plain: m_groups must be 1 or n_groups"):
        ctx.bfv_dot_plain(params, g0, g1, np.stack([m[:2]] * 2))
    # the term limit: before any pass over the inputs (the arrays here are far shorter than the counts)
    with pytest.raises(zk.ZkfheError, match=r"bfv_dot: n_terms %d is above the limit %d\b" % (limit + 1, limit)):
        dot(edge, 1, limit + 1, 1, w)
    with pytest.raises(zk.ZkfheError, match=r"bfv_dot_plain: n_terms %d is above the limit %d\b" % (limit_plain + 1, limit_plain)):
        plain(edge, 1, limit_plain + 1, 1)
    # ranges
    bad = a0.copy()
    bad[1, 7] = q
    with pytest.raises(zk.ZkfheError, match="bfv_dot: a ciphertext coefficient is not below Q"):
        ctx.bfv_dot(params, a0, bad, b0, b1, rlk0, rlk1, base_bits=w)
    with pytest.raises(zk.ZkfheError, match="bfv_dot: a ciphertext coefficient is not below Q"):
        ctx.bfv_dot(params, a0, a1, bad, b1, rlk0, rlk1, base_bits=w)
    with pytest.raises(zk.ZkfheError, match="bfv_dot_plain: a ciphertext coefficient is not below Q"):
        ctx.bfv_dot_plain(params, bad, a1, m[:2])
    bad_rlk = rlk1.copy()
    bad_rlk[0, 0] = 1 << 62
    with pytest.raises(zk.ZkfheError, match="bfv_dot: a relinearization-key coefficient is not below Q"):
        ctx.bfv_dot(params, a0, a1, b0, b1, rlk0, bad_rlk, base_bits=w)
    bad_m = m[:2].copy()
    bad_m[1, 3] = t // 2 + 1
    with pytest.raises(zk.ZkfheError, match="bfv_dot_plain: a plaintext coefficient is outside"):
        ctx.bfv_dot_plain(params, a0, a1, bad_m)
    # shapes
    with pytest.raises(ValueError, match="a0 and a1 must have the same shape"):
        ctx.bfv_dot(params, a0, a1[:1], b0, b1, rlk0, rlk1, base_bits=w)
    with pytest.raises(ValueError, match="a0 and a1 must have the same shape"):
        ctx.bfv_dot(params, a0[0], a1[0], b0, b1, rlk0, rlk1, base_bits=w)
    with pytest.raises(ValueError, match="b0 and b1 must hold the n_terms = 2"):
        ctx.bfv_dot(params, a0, a1, c0[1:], c1[1:], rlk0, rlk1, base_bits=w)
    with pytest.raises(ValueError, match="b0 and b1 must hold the n_terms = 2"):
        ctx.bfv_dot(params, a0, a1, g0, g1, rlk0, rlk1, base_bits=w)   # a 3-D b beside a 2-D a
    with pytest.raises(ValueError, match="rlk0 and rlk1"):
        ctx.bfv_dot(params, a0, a1, b0, b1, rlk0[:-1], rlk1[:-1], base_bits=w)
    with pytest.raises(ValueError, match="m must hold the n_terms = 2"):
        ctx.bfv_dot_plain(params, a0, a1, m[:3])
    # the context still works
    out0, out1 = ctx.bfv_dot(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    assert np.array_equal(ctx.bfv_decrypt(params, sk, out0, out1)[0], plain_dot(m[:2], m[2:], params))
