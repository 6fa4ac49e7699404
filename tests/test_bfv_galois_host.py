"""Host side of BFV slots and rotations (no GPU): pure-Python restatements of sigma_g, slot encoding (interpolation) and decoding
(evaluation), the Galois key and the key switch of zkfhe.h, with their properties at N = 16 (T = 97) and N = 1024 (T = 12289):
decode o encode = id, sigma_{5^k} rotates the rows by k, sigma_{2N-1} swaps them, the slot_sum composition totals the slots, and a
key switch decrypts to sigma_g(m).  Also the host-only calls against the restatements, their refusals, the declarations and
exports, and a slot-encoded ballot that the existing encryption circuit accepts.  tests/test_gpu_bfv_galois.py imports these
restatements."""
import json
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, circ, deg, kron_negacyclic, relin_digits
from tests.test_bfv_threshold_host import add, error, neg, ref_decrypt, ref_encrypt, ref_keygen_share, ring_mul, ternary, uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_slot_count", "zkfhe_bfv_galois_element", "zkfhe_bfv_slot_sum_elements", "zkfhe_bfv_encode_slots",
               "zkfhe_bfv_decode_slots", "zkfhe_bfv_galois_keygen", "zkfhe_bfv_apply_galois", "zkfhe_bfv_slot_sum", "zkfhe_bfv_galois_share"]
METHODS = ["bfv_encode_slots", "bfv_decode_slots", "bfv_galois_keygen", "bfv_apply_galois", "bfv_slot_sum", "bfv_galois_share"]


# ---- the definitions, restated from zkfhe.h --------------------------------------------------------------------------------

def sigma(v, g, q):
    """sigma_g of one polynomial of residues in CircuitInput order: coefficient i moves to k = i g mod 2N, negated at k - N past N"""
    d = deg(v)
    n = len(d)
    out = [0] * n
    for i, x in enumerate(d):
        k = i * g % (2 * n)
        if k < n:
            out[k] = x
        else:
            out[k - n] = -x
    return circ(out, q)


def is_prime(t):
    return t >= 2 and all(t % f for f in range(2, int(t ** 0.5) + 1))


def batching(n, t):
    return t < 1 << 31 and (t - 1) % (2 * n) == 0 and is_prime(t)


def primitive_root(t):
    f, rest, fs = 2, t - 1, []
    while f * f <= rest:
        if rest % f == 0:
            fs.append(f)
            while rest % f == 0:
                rest //= f
        f += 1
    if rest > 1:
        fs.append(rest)
    return next(r for r in range(2, t) if all(pow(r, (t - 1) // p, t) != 1 for p in fs))


def slot_exponents(n):
    """e_p of slot p = row N/2 + j: (-1)^row 5^j mod 2N"""
    e = [pow(5, j, 2 * n) for j in range(n // 2)]
    return e + [2 * n - x for x in e]


def _tables(n, t):
    z = pow(primitive_root(t), (t - 1) // (2 * n), t)
    zp = np.array([pow(z, k, t) for k in range(2 * n)], dtype=np.int64)
    return zp, np.array(slot_exponents(n), dtype=np.int64)


def plain_mod_t(m, q, t):
    """a plaintext (residues mod Q, CircuitInput order) -> its coefficients mod T in degree order"""
    return np.array([(int(x) - q) % t if int(x) > q // 2 else int(x) % t for x in deg(m)], dtype=np.int64)


def eval_slots(params, m, slots=None):
    """decode restated: the value of every slot (or of the listed ones) of the plaintext m, m(zeta^(e_p)) mod T"""
    n, q, t = params[0], params[1], params[2]
    zp, e = _tables(n, t)
    c, i = plain_mod_t(m, q, t), np.arange(n, dtype=np.int64)
    slots = range(n) if slots is None else slots
    return np.array([int((c * zp[(i * e[p]) % (2 * n)]).sum() % t) for p in slots], dtype=np.uint64)


def encode(params, values):
    """encode restated by interpolation: m_i = N^-1 sum_p v_p zeta^(-i e_p) mod T, centred, as residues mod Q"""
    n, q, t = params[0], params[1], params[2]
    zp, e = _tables(n, t)
    v, n_inv = np.asarray(values, dtype=np.int64), pow(n, t - 2, t)
    m = [int((v * zp[(-i * e) % (2 * n)]).sum() % t) * n_inv % t for i in range(n)]
    return circ([x - t if x > t // 2 else x for x in m], q)


def rotate(values, k, swap=False):
    """the slots after sigma_{5^k} (both rows left by k), then the row swap of sigma_{2N-1}"""
    v = np.asarray(values).reshape(2, -1)
    v = np.roll(v, -k, axis=1)
    return (v[::-1] if swap else v).reshape(-1)


def galois_element(n, steps=0, swap_rows=False):
    g = pow(5, steps % (n // 2), 2 * n)
    return g * (2 * n - 1) % (2 * n) if swap_rows else g


def slot_sum_elements(n):
    return [pow(5, 1 << k, 2 * n) for k in range(n.bit_length() - 2)] + [2 * n - 1]


def plain_slot_sum(params, m):
    """the slot_sum composition x <- x + sigma_g(x) on a plaintext, mod T (what the ciphertext result decrypts to)"""
    n, q, t = params[0], params[1], params[2]
    x = [int(v) for v in plain_mod_t(m, q, t)]
    for g in slot_sum_elements(n):
        s = [int(v) for v in plain_mod_t(sigma(circ(x, t), g, t), t, t)]
        x = [(a + b) % t for a, b in zip(x, s)]
    return circ([v - t if v > t // 2 else v for v in x], q)


def ref_galois_key(params, s, crs_seed, party_seed, g, w):
    """rows r_j = -(a_j s + e_j) + 2^(j w) sigma_g(s) mod Q and a_j: a_j from (crs_seed, 14, g 64 + j), e_j from (party_seed, 15, ...)"""
    n, q, b = params[0], params[1], params[3]
    ss = sigma(s, g, q)
    r, a = [], []
    for j in range(relin_digits(q, w)):
        aj = uniform(crs_seed, 14, g * 64 + j, n, q)
        ej = error(party_seed, 15, g * 64 + j, n, q, b)
        gadget = np.array([int(x) * (1 << (j * w)) % q for x in ss], dtype=np.uint64)
        r.append(add(neg(add(ring_mul(aj, s, q), ej, q=q), q), gadget, q=q))
        a.append(aj)
    return np.array(r), np.array(a)


def ref_apply_galois(params, c0, c1, g, gk0, gk1, w):
    """zkfhe_bfv_apply_galois of one ciphertext restated: digits of sigma_g(c1), exact sums over Z, then mod Q"""
    n, q = params[0], params[1]
    s0, s1 = sigma(c0, g, q), deg(sigma(c1, g, q))
    l = relin_digits(q, w)
    digits = [[(c >> (i * w)) & ((1 << w) - 1) for c in s1] for i in range(l)]
    k0 = kron_negacyclic([(digits[i], deg(gk0[i])) for i in range(l)], n)
    k1 = kron_negacyclic([(digits[i], deg(gk1[i])) for i in range(l)], n)
    return circ([x + y for x, y in zip(deg(s0), k0)], q), circ(k1, q)


# ---- tests -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,t", [(16, 97), (1024, 12289)])
def test_encode_decode_rotations_and_slot_sum_restated(n, t):
    params = (n, Q60, t, 19)
    q = params[1]
    rng = random.Random(n)
    v = np.array([rng.randrange(t) for _ in range(n)], dtype=np.uint64)
    m = encode(params, v)
    assert all(int(x) <= t // 2 or int(x) >= q - t // 2 for x in m)
    assert np.array_equal(eval_slots(params, m), v)
    for k in (1, 3, -1, n // 2 - 2):
        assert np.array_equal(eval_slots(params, sigma(m, galois_element(n, k), q)), rotate(v, k % (n // 2))), k
    assert np.array_equal(eval_slots(params, sigma(m, 2 * n - 1, q)), rotate(v, 0, swap=True))
    assert np.array_equal(eval_slots(params, sigma(m, galois_element(n, 2, True), q)), rotate(v, 2, swap=True))
    total = int(v.astype(object).sum()) % t
    assert np.array_equal(eval_slots(params, plain_slot_sum(params, m)), np.full(n, total, dtype=np.uint64))


def test_sigma_composes_and_has_inverse():
    n, q = 16, Q29
    v = uniform(b"\x07" * 32, 5, 0, n, q)
    for g, h in ((5, 13), (3, 31), (7, 9)):
        assert np.array_equal(sigma(sigma(v, g, q), h, q), sigma(v, g * h % (2 * n), q))
    assert np.array_equal(sigma(v, 1, q), v)
    assert np.array_equal(sigma(sigma(v, 5, q), pow(5, -1, 2 * n), q), v)


@pytest.mark.parametrize("params,w", [((16, Q29, 97, 19), 4), ((16, Q60, 97, 19), 16)])
def test_key_switch_decrypts_to_sigma_restated(params, w):
    n, q, t = params[0], params[1], params[2]
    s, pk0, pk1 = ref_keygen_share(params, b"\x21" * 32, b"\x21" * 32)
    v = np.array([random.Random(1).randrange(t) for _ in range(n)], dtype=np.uint64)
    m = encode(params, v)
    c0, c1 = ref_encrypt(params, pk0, pk1, m, b"\x22" * 32, 0)
    for g in (1, 5, 2 * n - 1, galois_element(n, 3)):
        gk0, gk1 = ref_galois_key(params, s, b"\x23" * 32, b"\x23" * 32, g, w)
        o0, o1 = ref_apply_galois(params, c0, c1, g, gk0, gk1, w)
        got = ref_decrypt(params, s, o0, o1)[0]
        assert np.array_equal(got, sigma(m, g, q)), g
    g = galois_element(n, 3)
    assert np.array_equal(eval_slots(params, sigma(m, g, q)), rotate(v, 3))


def test_host_calls_match_restatement():
    for n, t in ((16, 97), (1024, 12289), (4096, 65537), (32768, 65537)):
        params = (n, Q60, t, 19)
        assert zk.bfv_slot_count(params) == n
        assert zk.bfv_slot_sum_elements(params) == slot_sum_elements(n)
        for steps in (0, 1, 2, 7, n // 2 - 1, n // 2, n // 2 + 3, -1, -5, -n, 10 ** 12, -(10 ** 12)):
            for swap in (False, True):
                assert zk.bfv_galois_element(params, steps, swap) == galois_element(n, steps, swap), (n, steps, swap)
    assert zk.bfv_galois_element((16, Q29, 97, 19), 0, True) == 31
    assert zk.bfv_slot_sum_elements((8, Q29, 7, 19)) == [5, 9, 15]   # defined for any T
    assert zk.bfv_galois_element((8, Q29, 7, 19), 1) == 5


@pytest.mark.parametrize("n,t", [(1024, 7), (1024, 6145), (1024, 13313), (16, 65), (16, 161)])
def test_slot_count_refuses_non_batching_t(n, t):
    assert not batching(n, t)
    with pytest.raises(zk.ZkfheError, match="batching"):
        zk.bfv_slot_count((n, Q60, t, 19))


def test_host_calls_refuse_bad_params():
    for fn in (zk.bfv_slot_count, zk.bfv_slot_sum_elements, zk.bfv_galois_element):
        with pytest.raises(zk.ZkfheError, match="bfv params"):
            fn((12, Q29, 97, 19))
    assert batching(2048, 12289) and not batching(4096, 12289) and batching(32768, 65537)


def test_slot_encoded_ballot_passes_the_circuit():
    """a ballot encoded by the restatement and encrypted by the restated zkfhe_bfv_encrypt satisfies the existing circuit"""
    from tests.test_gpu_bfv_encrypt import to_json
    params = (1024, Q29, 12289, 19)
    n, q, t, b = params
    seed, enc_seed = b"\x31" * 32, b"\x32" * 32
    _, pk0, pk1 = ref_keygen_share(params, seed, seed)
    votes = np.zeros(n, dtype=np.uint64)
    votes[[0, 3, 7, n // 2 + 1]] = 1
    votes[5] = t - 1
    m = encode(params, votes)
    c0, c1 = ref_encrypt(params, pk0, pk1, m, enc_seed, 0)
    ct = dict(u=[ternary(enc_seed, 1, 0, n, q)], e0=[error(enc_seed, 2, 0, n, q, b)], e1=[error(enc_seed, 3, 0, n, q, b)], c0=[c0], c1=[c1])
    text = to_json(pk0, pk1, m, ct)
    cfg = zk.bfv_auto_config(text, params, 13)
    fails, first = zk.bfv_mock(text, params, cfg)
    assert fails == 0, first
    assert json.loads(text)["m"] == [str(int(x)) for x in m]


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    for name in METHODS:
        assert callable(getattr(zk.Context, name)), name
    for name in ("bfv_slot_count", "bfv_galois_element", "bfv_slot_sum_elements"):
        assert callable(getattr(zk, name)), name
    for word in ("domain 14", "domain 15", "g 64 + ", "SEED IS SECRET", "2^w"):
        assert word in header, word
    assert zk.PROF_BFV_GALOIS == 14 and zk.PROF_BFV_SLOT_NTT == 15
    assert re.search(r"#define ZKFHE_PROF_BFV_GALOIS 14\b", header) and re.search(r"#define ZKFHE_PROF_BFV_SLOT_NTT 15\b", header)
