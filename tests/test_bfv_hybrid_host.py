"""Hybrid key switching without a GPU (zkfhe.h "Evaluation keys modulo Q P: hybrid key switching"): the definitions restated on
Python integers (the keys from their seeds with oracle/chacha20_ref.py behind the samplers of tests/test_bfv_threshold_host.py, the
key switch with its division by P, and mul, dot, apply_galois, slot_sum and pack on top of it), the decryption and the noise bound of
the restated key switch, zkfhe_bfv_hybrid_max_p against its formula, the declarations and exports, and the refusals that need no
device.  tests/test_gpu_bfv_hybrid.py imports the restatement."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, Q63, centred, circ, deg, kron_negacyclic, ref_tensor, relin_digits
from tests.test_bfv_galois_host import sigma, slot_sum_elements
from tests.test_bfv_pack_host import monomial, prepare, sub
from tests.test_bfv_threshold_host import add, error, ref_decrypt, ref_encrypt, ref_keygen_share, ref_noise, uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_hybrid_max_p", "zkfhe_bfv_relin_keygen_hybrid", "zkfhe_bfv_galois_share_hybrid", "zkfhe_bfv_galois_keygen_hybrid",
               "zkfhe_bfv_evk_create_hybrid", "zkfhe_bfv_evk_special_modulus"]
P5 = 2013265921 * 469762049 * 754974721 * 2147352577 * 2146959361
K13 = (1024, Q29, 7, 19)
P30 = (1 << 30) - 35   # a 30-bit odd number
KEY_SEED, ENC_SEED, GK_SEED = b"\x81" * 32, b"\x82" * 32, b"\x83" * 32


# ---- the definitions, restated from zkfhe.h --------------------------------------------------------------------------------

def max_p(params, w):
    """the largest P below 2^63 with l N (2^w - 1) (Q P - 1) <= floor(P5 / 2)"""
    n, q = params[0], params[1]
    return min(((P5 // 2) // (relin_digits(q, w) * n * ((1 << w) - 1)) + 1) // q, (1 << 63) - 1)


def bound_holds(params, w, p):
    n, q = params[0], params[1]
    return relin_digits(q, w) * n * ((1 << w) - 1) * (q * p - 1) <= P5 // 2


def ref_hybrid_key(params, p, s, crs_seed, party_seed, g, w):
    """the four planes (r_q, a_q, r_p, a_p), each (l, N), of the relinearization key (g None: gadget s^2, domains 7, 8, 23, index i)
    or of the Galois key of g (gadget sigma_g(s), domains 14, 15, 24, index g 64 + i): r_q = -(aQ s + e) + (P mod Q) 2^(i w) G mod Q,
    r_p = -(aP s + e) mod P with the same centred e"""
    n, q, b = params[0], params[1], params[3]
    sc = centred(deg(s), q)
    gadget = kron_negacyclic([(sc, sc)], n) if g is None else centred(deg(sigma(s, g, q)), q)
    dom_a, dom_e, dom_ap, index0 = (7, 8, 23, 0) if g is None else (14, 15, 24, g * 64)
    planes = [[], [], [], []]
    for i in range(relin_digits(q, w)):
        aq, ap = uniform(crs_seed, dom_a, index0 + i, n, q), uniform(crs_seed, dom_ap, index0 + i, n, p)
        e = centred(deg(error(party_seed, dom_e, index0 + i, n, q, b)), q)
        xq, xp = kron_negacyclic([(deg(aq), sc)], n), kron_negacyclic([(deg(ap), sc)], n)
        planes[0].append(circ([-(x + y) + (p % q) * (1 << (i * w)) * z for x, y, z in zip(xq, e, gadget)], q))
        planes[1].append(aq)
        planes[2].append(circ([-(x + y) for x, y in zip(xp, e)], p))
        planes[3].append(ap)
    return tuple(np.array(x) for x in planes)


def lift(kq, kp, q, p):
    """the integers below Q P of one key row (degree order) from its planes"""
    q_inv = pow(q, -1, p)
    return [a + q * ((b - a) * q_inv % p) for a, b in zip(deg(kq), deg(kp))]


def ref_hybrid_switch(params, p, v, key, w):
    """the hybrid key switch of the source v (degree order, integers in [0, Q)) with key = (k0_q, k1_q, k0_p, k1_p): r_0, r_1 in
    degree order, r_j = floor((2 X_j + P) / 2P) mod Q of X_j = sum_i d_i Kj_i over Z"""
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    digits = [[(c >> (i * w)) & ((1 << w) - 1) for c in v] for i in range(l)]
    out = []
    for j in range(2):
        x = kron_negacyclic([(digits[i], lift(key[j][i], key[2 + j][i], q, p)) for i in range(l)], n)
        out.append([(2 * c + p) // (2 * p) % q for c in x])
    return out


def ref_mul_hybrid(params, p, a0, a1, b0, b1, rlk, w):
    """zkfhe_bfv_mul of one pair with a hybrid relinearization key"""
    q = params[1]
    c0, c1, c2 = ref_tensor(params, a0, a1, b0, b1)
    r0, r1 = ref_hybrid_switch(params, p, c2, rlk, w)
    return circ([x + y for x, y in zip(c0, r0)], q), circ([x + y for x, y in zip(c1, r1)], q)


def ref_dot_hybrid(params, p, a0, a1, b0, b1, rlk, w):
    """zkfhe_bfv_dot of one group (a0, a1, b0, b1 of shape (n_terms, N)) with a hybrid relinearization key"""
    n, q, t = params[0], params[1], params[2]
    A0, A1, B0, B1 = ([centred(deg(row), q) for row in x] for x in (a0, a1, b0, b1))
    terms = range(len(A0))
    xs = (kron_negacyclic([(A0[i], B0[i]) for i in terms], n),
          kron_negacyclic([(A0[i], B1[i]) for i in terms] + [(A1[i], B0[i]) for i in terms], n),
          kron_negacyclic([(A1[i], B1[i]) for i in terms], n))
    c0, c1, c2 = ([(2 * t * x + q) // (2 * q) % q for x in xj] for xj in xs)
    r0, r1 = ref_hybrid_switch(params, p, c2, rlk, w)
    return circ([x + y for x, y in zip(c0, r0)], q), circ([x + y for x, y in zip(c1, r1)], q)


def ref_apply_galois_hybrid(params, p, c0, c1, g, gk, w):
    """zkfhe_bfv_apply_galois of one ciphertext with a hybrid key for g"""
    q = params[1]
    r0, r1 = ref_hybrid_switch(params, p, deg(sigma(c1, g, q)), gk, w)
    return circ([x + y for x, y in zip(deg(sigma(c0, g, q)), r0)], q), circ(r1, q)


def ref_slot_sum_hybrid(params, p, c0, c1, gks, w):
    """zkfhe_bfv_slot_sum of one ciphertext: x <- x + apply_galois(x, g) over slot_sum_elements, gks[k] the hybrid key of element k"""
    q = params[1]
    for g, gk in zip(slot_sum_elements(params[0]), gks):
        y0, y1 = ref_apply_galois_hybrid(params, p, c0, c1, g, gk, w)
        c0, c1 = add(c0, y0, q=q), add(c1, y1, q=q)
    return c0, c1


def ref_pack_hybrid(params, p, c0, c1, pos, gks, w):
    """zkfhe_bfv_pack of one group in the level form of tests/test_bfv_pack_host.py (ref_pack), gks[lv - 1] the hybrid key of
    2^lv + 1"""
    n_ring, q = params[0], params[1]

    def step(e, o, lv):
        if o is None:
            total, diff = e, e
        else:
            t = [monomial(c, n_ring >> lv, q) for c in o]
            total, diff = [add(a, b, q=q) for a, b in zip(e, t)], [sub(a, b, q) for a, b in zip(e, t)]
        k0, k1 = ref_apply_galois_hybrid(params, p, diff[0], diff[1], (1 << lv) + 1, gks[lv - 1], w)
        return add(total[0], k0, q=q), add(total[1], k1, q=q)

    wi = prepare(params, c0, c1, [0] * len(c0) if pos is None else pos)
    levels = len(wi).bit_length() - 1
    for lv in range(1, levels + 1):
        h = len(wi) >> 1
        wi = [step(wi[i], wi[i + h], lv) for i in range(h)]
    for lv in range(levels + 1, n_ring.bit_length()):
        wi = [step(wi[0], None, lv)]
    return wi[0]


def switch_noise_bound(params, w, p):
    """what one hybrid key switch adds under a single ternary key: with E = sum_i d_i e_i, r_0 + r_1 s = v s' + E / P + rho_0 +
    rho_1 s with |rho| <= 1/2 per coefficient, so at most ceil(l N (2^w - 1) B / P) + (N + 1) / 2"""
    n, q, b = params[0], params[1], params[3]
    return -(-(relin_digits(q, w) * n * ((1 << w) - 1) * b) // p) + (n + 1) // 2


def plain(rng, params):
    n, q, t = params[0], params[1], params[2]
    return np.array([rng.randrange(-(t // 2), t // 2 + 1) % q for _ in range(n)], dtype=np.uint64)


# ---- tests -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [(16, Q29, 7, 19), K13], ids=["N16", "N1024"])
@pytest.mark.parametrize("w", [8, 16])
def test_restated_key_switch_decrypts_and_keeps_the_bound(params, w):
    n, q = params[0], params[1]
    rng = random.Random(n + w)
    s, pk0, pk1 = ref_keygen_share(params, KEY_SEED, KEY_SEED)
    m = plain(rng, params)
    c0, c1 = ref_encrypt(params, pk0, pk1, m, ENC_SEED, 0)
    fresh = ref_noise(params, s, c0, c1, m)
    g = 5
    for p in (P30, max_p(params, w) - (1 - max_p(params, w) % 2)):   # a 30-bit P and the largest odd admissible one
        assert bound_holds(params, w, p)
        gk = ref_hybrid_key(params, p, s, GK_SEED, GK_SEED, g, w)
        r0, r1 = ref_apply_galois_hybrid(params, p, c0, c1, g, gk, w)
        want = sigma(m, g, q)
        assert np.array_equal(ref_decrypt(params, s, r0, r1)[0], want)
        assert ref_noise(params, s, r0, r1, want) <= fresh + switch_noise_bound(params, w, p)


def test_restated_relinearization_decrypts():
    params, w, p = (16, Q60, 97, 19), 16, P30
    n, q, t = params[0], params[1], params[2]
    rng = random.Random(5)
    s, pk0, pk1 = ref_keygen_share(params, KEY_SEED, KEY_SEED)
    ma, mb = plain(rng, params), plain(rng, params)
    a, b = ref_encrypt(params, pk0, pk1, ma, ENC_SEED, 0), ref_encrypt(params, pk0, pk1, mb, ENC_SEED, 1)
    rlk = ref_hybrid_key(params, p, s, GK_SEED, GK_SEED, None, w)
    r0, r1 = ref_mul_hybrid(params, p, *a, *b, rlk, w)
    prod = kron_negacyclic([(centred(deg(ma), q), centred(deg(mb), q))], n)
    want = circ([x % t - t if x % t > t // 2 else x % t for x in prod], q)
    assert np.array_equal(ref_decrypt(params, s, r0, r1)[0], want)
    d0, d1 = ref_dot_hybrid(params, p, np.array([a[0]]), np.array([a[1]]), np.array([b[0]]), np.array([b[1]]), rlk, w)
    assert np.array_equal(d0, r0) and np.array_equal(d1, r1)   # one term: the product


@pytest.mark.parametrize("params,w", [(K13, 4), (K13, 8), (K13, 29), ((4096, Q60, 65537, 19), 16), ((32768, Q63, 65537, 19), 32),
                                      ((8, 1 << 16, 7, 19), 8), ((32768, Q63, 65537, 19), 1)])
def test_hybrid_max_p_matches_its_formula(params, w):
    got = zk.bfv_hybrid_max_p(params, w)
    assert got == max_p(params, w) and got >= 1 << 34
    assert bound_holds(params, w, got)
    assert got == (1 << 63) - 1 or not bound_holds(params, w, got + 1)


def test_hybrid_max_p_refusals():
    with pytest.raises(zk.ZkfheError, match="bfv_hybrid_max_p: base_bits"):
        zk.bfv_hybrid_max_p(K13, 0)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        zk.bfv_hybrid_max_p((12, Q29, 7, 19), 8)
    lib = zk.load_library()
    prm = zk.BfvParamsC(*K13)
    assert lib.zkfhe_bfv_hybrid_max_p(ctypes.byref(prm), 8, None) != 0
    assert lib.zkfhe_last_error(None).decode() == "bfv_hybrid_max_p: p_max is NULL"


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zk.EXPORTS and hasattr(lib, name)
    assert "domain 23" in header and "domain 24" in header


def test_python_methods_exist():
    assert callable(zk.bfv_hybrid_max_p)
    for name in ("bfv_relin_keygen_hybrid", "bfv_galois_keygen_hybrid", "bfv_galois_share_hybrid", "bfv_evk_hybrid"):
        assert callable(getattr(zk.Context, name)), name
    assert isinstance(zk.BfvEvalKeys.special_modulus, property)


def test_calls_without_a_context_are_refused_before_any_device_work():
    lib = zk.load_library()
    prm = zk.BfvParamsC(8, Q29, 7, 19)
    none = [None] * 4
    calls = [("zkfhe_bfv_relin_keygen_hybrid", [None, ctypes.byref(prm), P30, None, None, 8] + none),
             ("zkfhe_bfv_galois_keygen_hybrid", [None, ctypes.byref(prm), P30, None, None, 5, 8] + none),
             ("zkfhe_bfv_galois_share_hybrid", [None, ctypes.byref(prm), P30, None, None, None, 5, 8] + none)]
    for name, args in calls:
        assert getattr(lib, name)(*args) != 0, name
    out = ctypes.c_void_p(1)
    assert lib.zkfhe_bfv_evk_create_hybrid(None, ctypes.byref(prm), P30, 8, *none, 0, None, *none, ctypes.byref(out)) != 0
    assert out.value is None and lib.zkfhe_last_error(None).decode() == "bfv_evk_create_hybrid: a NULL argument or a zero count"
    assert lib.zkfhe_bfv_evk_special_modulus(None, None) != 0
    assert lib.zkfhe_last_error(None).decode() == "bfv_evk_special_modulus: a NULL argument"
