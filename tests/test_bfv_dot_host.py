"""Host side of the fused BFV inner products (no GPU): the declarations and exports of the new entry points, the oracles ref_dot and
ref_dot_plain restated from the definitions of zkfhe.h (tests/test_gpu_bfv_dot.py imports them), the term limit against its
big-integer formula, and the noise margin that the GPU decryption test relies on."""
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, Q63, centred, circ, deg, kron_negacyclic, ref_mul, relin_digits, schoolbook_negacyclic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_dot_max_terms", "zkfhe_bfv_dot", "zkfhe_bfv_dot_plain"]
P5 = 2013265921 * 469762049 * 754974721 * 2147352577 * 2146959361   # the five RNS primes of rns_ntt.hip.hpp
SIZE_MAX = (1 << 64) - 1


# ---- the oracles -------------------------------------------------------------------------------------------------------------

def ref_dot(params, a0, a1, b0, b1, rlk0, rlk1, w):
    """zkfhe_bfv_dot of one group, restated from its definition (zkfhe.h): a0, a1, b0, b1 of shape (n_terms, N); CircuitInput order
    in and out"""
    n, q, t = params[0], params[1], params[2]
    A0, A1, B0, B1 = ([centred(deg(row), q) for row in x] for x in (a0, a1, b0, b1))
    terms = range(len(A0))
    xs = (kron_negacyclic([(A0[i], B0[i]) for i in terms], n),
          kron_negacyclic([(A0[i], B1[i]) for i in terms] + [(A1[i], B0[i]) for i in terms], n),
          kron_negacyclic([(A1[i], B1[i]) for i in terms], n))
    c0, c1, c2 = ([(2 * t * x + q) // (2 * q) % q for x in xj] for xj in xs)
    l = relin_digits(q, w)
    digits = [[(c >> (i * w)) & ((1 << w) - 1) for c in c2] for i in range(l)]
    s0 = kron_negacyclic([(digits[i], deg(rlk0[i])) for i in range(l)], n)
    s1 = kron_negacyclic([(digits[i], deg(rlk1[i])) for i in range(l)], n)
    return circ([x + y for x, y in zip(c0, s0)], q), circ([x + y for x, y in zip(c1, s1)], q)


def ref_dot_plain(params, c0, c1, m):
    """zkfhe_bfv_dot_plain of one group: sum_i c_j,i m_i mod (x^N + 1, Q); c0, c1, m of shape (n_terms, N)"""
    n, q = params[0], params[1]
    C0, C1, M = ([centred(deg(row), q) for row in x] for x in (c0, c1, m))
    terms = range(len(M))
    return (circ(kron_negacyclic([(C0[i], M[i]) for i in terms], n), q), circ(kron_negacyclic([(C1[i], M[i]) for i in terms], n), q))


def max_terms(params, plain):
    """zkfhe_bfv_dot_max_terms from its formula on Python integers"""
    n, q, t = params[0], params[1], params[2]
    per_term = n * (q // 2) * (t // 2) if plain else 2 * n * (q // 2) ** 2
    return min((P5 // 2) // per_term, SIZE_MAX)


def host_relin_key(sk, q, w, b, rng):
    """the relinearization key of zkfhe.h for a ternary sk (degree order, values in {-1, 0, 1}): rlk0_i = -(a_i s + e_i) + 2^(i w) s^2,
    rlk1_i = a_i, as (l, N) arrays in CircuitInput order"""
    from zk_fhe_amd import inputs
    n = len(sk)
    s = [int(x) for x in sk]
    s2 = kron_negacyclic([(s, s)], n)
    rlk0, rlk1 = [], []
    for i in range(relin_digits(q, w)):
        a = rng.integers(0, q, n, dtype=np.int64)
        e = inputs._chi_error(rng, n, b)
        a_s = inputs._negacyclic_ternary(a, sk, q)
        rlk0.append(circ([(1 << (i * w)) * int(x) - int(y) - int(z) for x, y, z in zip(s2, a_s, e)], q))
        rlk1.append(circ([int(x) for x in a], q))
    return np.array(rlk0), np.array(rlk1)


def host_noise(sk, out0, out1, want_m, q, t):
    """max |[out0 + out1 s - floor(Q/T) m]_Q| for the expected plaintext m (degree order, centred); sk in degree order"""
    n = len(sk)
    c1s = kron_negacyclic([(deg(out1), [int(x) for x in sk])], n)
    worst = 0
    for x0, x1, m in zip(deg(out0), c1s, want_m):
        e = (x0 + x1 - (q // t) * m) % q
        worst = max(worst, q - e if e > q // 2 else e)
    return worst


# ---- tests -------------------------------------------------------------------------------------------------------------------

def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    assert re.search(r"#define ZKFHE_PROF_BFV_DOT 20\b", header) and zk.PROF_BFV_DOT == 20
    for name in ("bfv_dot", "bfv_dot_plain"):
        assert callable(getattr(zk.Context, name)), name
    assert callable(zk.bfv_dot_max_terms)
    assert str(P5) in header


def small_case():
    params, w, terms = (8, 97, 5, 1), 3, 3
    rng = random.Random(11)
    pick = lambda rows: np.array([[rng.randrange(97) for _ in range(8)] for _ in range(rows)], dtype=np.uint64)  # noqa: E731
    l = relin_digits(97, w)
    return params, w, pick(terms), pick(terms), pick(terms), pick(terms), pick(l), pick(l)


def test_reference_dot_small_case():
    # the definition on a hand-sized case: N = 8, Q = 97, T = 5, w = 3, 3 terms, against schoolbook sums
    params, w, a0, a1, b0, b1, rlk0, rlk1 = small_case()
    n, q, t = params[0], params[1], params[2]
    out0, out1 = ref_dot(params, a0, a1, b0, b1, rlk0, rlk1, w)
    A0, A1, B0, B1 = ([centred(deg(r), q) for r in x] for x in (a0, a1, b0, b1))

    def total(pairs):
        acc = [0] * n
        for x, y in pairs:
            acc = [u + v for u, v in zip(acc, schoolbook_negacyclic(x, y))]
        return acc

    x0 = total(zip(A0, B0))
    x1 = total(list(zip(A0, B1)) + list(zip(A1, B0)))
    x2 = total(zip(A1, B1))
    rnd = lambda xs: [(2 * t * x + q) // (2 * q) % q for x in xs]  # noqa: E731
    c0, c1, c2 = rnd(x0), rnd(x1), rnd(x2)
    l = relin_digits(q, w)
    assert l == 3
    d = [[(c >> (w * i)) & 7 for c in c2] for i in range(l)]
    s0 = total((d[i], deg(rlk0[i])) for i in range(l))
    s1 = total((d[i], deg(rlk1[i])) for i in range(l))
    assert np.array_equal(out0, circ([u + v for u, v in zip(c0, s0)], q))
    assert np.array_equal(out1, circ([u + v for u, v in zip(c1, s1)], q))
    assert out0.dtype == np.uint64 and out0.shape == (n,)
    # the sum rounds once: it is not the sum of the rounded products (the case would be too weak otherwise)
    parts = [ref_mul(params, a0[i], a1[i], b0[i], b1[i], rlk0, rlk1, w) for i in range(3)]
    assert not np.array_equal(out0.astype(object), sum(p[0].astype(object) for p in parts) % q)


def test_reference_dot_plain_small_case():
    params, w, c0, c1, _, _, _, _ = small_case()
    n, q, t = params[0], params[1], params[2]
    rng = random.Random(12)
    m = np.array([[rng.randrange(-(t // 2), t // 2 + 1) % q for _ in range(n)] for _ in range(3)], dtype=np.uint64)
    out0, out1 = ref_dot_plain(params, c0, c1, m)
    for got, c in ((out0, c0), (out1, c1)):
        acc = [0] * n
        for i in range(3):
            acc = [u + v for u, v in zip(acc, schoolbook_negacyclic(centred(deg(c[i]), q), centred(deg(m[i]), q)))]
        assert np.array_equal(got, circ(acc, q))


def test_reference_dot_of_one_term_is_reference_mul():
    params, w, a0, a1, b0, b1, rlk0, rlk1 = small_case()
    for i in range(3):
        got = ref_dot(params, a0[i:i + 1], a1[i:i + 1], b0[i:i + 1], b1[i:i + 1], rlk0, rlk1, w)
        want = ref_mul(params, a0[i], a1[i], b0[i], b1[i], rlk0, rlk1, w)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("params", [(1024, Q29, 7, 19), (4096, Q60, 65537, 19), (32768, Q63, Q63 - 2, 1), (8, 97, 5, 1), (8, Q63, 2, 1),
                                    (32768, Q60, 65537, 19)])
def test_max_terms_matches_the_formula(params):
    for plain in (False, True):
        assert zk.bfv_dot_max_terms(params, plain) == max_terms(params, plain), plain


def test_max_terms_values_and_refusals():
    assert zk.bfv_dot_max_terms((1024, Q29, 7, 19)) == SIZE_MAX            # saturates: 2^83 terms would fit
    assert zk.bfv_dot_max_terms((1024, Q29, 7, 19), plain=True) == SIZE_MAX
    edge = zk.bfv_dot_max_terms((32768, Q63, Q63 - 2, 1))
    assert 1000 < edge < 1300 and edge == (P5 // 2) // (2 * 32768 * (Q63 // 2) ** 2)
    # one more term passes half of the primes' product
    assert edge * 2 * 32768 * (Q63 // 2) ** 2 <= P5 // 2 < (edge + 1) * 2 * 32768 * (Q63 // 2) ** 2
    assert zk.bfv_dot_max_terms((4096, Q60, 65537, 19)) < SIZE_MAX
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        zk.bfv_dot_max_terms((1000, Q60, 65537, 19))


@pytest.mark.parametrize("seed", [1, 2])
def test_noise_margin_of_sixteen_terms(seed):
    """The GPU decryption test sums 16 products at (1024, Q29, 7, 19) with w = 8 and asserts noise below floor(Q/T) / 2.  Here the
    same computation on the host (keygen and encrypt of zk_fhe_amd.inputs, ref_dot) must stay below floor(Q/T) / 8: a factor 4 under
    the decryption bound.  If a seed fails this, 16 terms are too many for the GPU test: lower both counts, never the bound."""
    from zk_fhe_amd import inputs
    n, q, t, b = 1024, Q29, 7, 19
    params, w, terms = (n, q, t, b), 8, 16
    rng = np.random.default_rng(seed)
    sk, pk = inputs.keygen(n, q, b, rng)
    rlk0, rlk1 = host_relin_key(sk, q, w, b, rng)
    ms = rng.integers(-(t // 2), t // 2 + 1, (2 * terms, n), dtype=np.int64)
    cts = [inputs.encrypt(pk, m, q, t, b, rng) for m in ms]
    c0 = np.array([circ([int(x) for x in ct["c0"]], q) for ct in cts])
    c1 = np.array([circ([int(x) for x in ct["c1"]], q) for ct in cts])
    out0, out1 = ref_dot(params, c0[:terms], c1[:terms], c0[terms:], c1[terms:], rlk0, rlk1, w)
    prod = kron_negacyclic([([int(x) for x in ms[i]], [int(x) for x in ms[terms + i]]) for i in range(terms)], n)
    want = [v % t - t if v % t > t // 2 else v % t for v in prod]
    noise = host_noise(sk, out0, out1, want, q, t)
    assert noise < (q // t) // 8, noise
    got = inputs.decrypt(sk, np.array(deg(out0), dtype=np.int64), np.array(deg(out1), dtype=np.int64), q, t)
    assert [int(x) for x in got] == want
