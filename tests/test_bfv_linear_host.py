"""Host side of hoisted BFV rotations and slot-wise linear transforms (no GPU): pure-Python restatements of the hoisted rotation and
of zkfhe_bfv_linear_transform from zkfhe.h, on the helpers of the other host tests.  At N = 16 (T = 97) every hoisted rotation
decrypts to sigma_g(m) without being bit-equal to zkfhe_bfv_apply_galois, and the transform decrypts to sum_k d_k[p] rot_k(v)[p];
the index rule of the NTT domain against a small negacyclic NTT written here; bfv_matrix_diagonals against matrix @ v; the
declarations, exports and mirrors.  tests/test_gpu_bfv_linear.py imports these restatements."""
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, centred, circ, deg, kron_negacyclic, relin_digits
from tests.test_bfv_galois_host import encode, eval_slots, galois_element, ref_apply_galois, ref_galois_key, rotate, sigma
from tests.test_bfv_threshold_host import ref_decrypt, ref_encrypt, ref_keygen_share, ref_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_apply_galois_many", "zkfhe_bfv_linear_transform"]
METHODS = ["bfv_apply_galois_many", "bfv_linear_transform"]


# ---- the definitions, restated from zkfhe.h --------------------------------------------------------------------------------

def sigma_z(d, g):
    """sigma_g of a signed integer polynomial in degree order: the coefficient of x^j moves to j g mod 2N, negated over Z past N"""
    n = len(d)
    out = [0] * n
    for j, x in enumerate(d):
        k = j * g % (2 * n)
        if k < n:
            out[k] = x
        else:
            out[k - n] = -x
    return out


def ref_hoisted_rotation(params, c0, c1, g, gk0, gk1, w):
    """the hoisted rotation of one ciphertext by g: digits of c1 itself, sigma_g on the integer digits, exact sums, then mod Q"""
    n, q = params[0], params[1]
    if g == 1:
        return np.array(c0, dtype=np.uint64), np.array(c1, dtype=np.uint64)
    l, d1 = relin_digits(q, w), deg(c1)
    digits = [sigma_z([(c >> (i * w)) & ((1 << w) - 1) for c in d1], g) for i in range(l)]
    k0 = kron_negacyclic([(digits[i], deg(gk0[i])) for i in range(l)], n)
    k1 = kron_negacyclic([(digits[i], deg(gk1[i])) for i in range(l)], n)
    return circ([x + y for x, y in zip(deg(sigma(c0, g, q)), k0)], q), circ(k1, q)


def ref_linear_transform(params, c0, c1, elements, gk0, gk1, w, diag):
    """zkfhe_bfv_linear_transform of one ciphertext: out = sum_k r_k p_k exactly over Z (p_k the centred diagonal), then mod Q"""
    n, q = params[0], params[1]
    rot = [ref_hoisted_rotation(params, c0, c1, g, gk0[k], gk1[k], w) for k, g in enumerate(elements)]
    p = [centred(deg(d), q) for d in diag]
    return tuple(circ(kron_negacyclic([(deg(r[j]), pk) for r, pk in zip(rot, p)], n), q) for j in (0, 1))


def transform_slots(params, v, elements, d):
    """sum_k d_k[p] rot_k(v)[p] mod T for elements = [(steps, swap)], on slot values"""
    t = params[2]
    out = np.zeros(params[0], dtype=object)
    for (steps, swap), dk in zip(elements, d):
        out = (out + np.asarray(dk, dtype=object) * np.asarray(rotate(v, steps, swap), dtype=object)) % t
    return out.astype(np.uint64)


def small_ntt(d, n, p, psi):
    """the merged-twist Cooley-Tukey transform of rns_forward on degree-order integers (fw[k] = psi^br(k)); index k ends as the
    evaluation at psi^(2 br(k) + 1)"""
    log_n = n.bit_length() - 1
    br = lambda k, bits: int(format(k, "0%db" % bits)[::-1], 2) if bits else 0  # noqa: E731
    fw = [pow(psi, br(k, log_n), p) for k in range(n)]
    a = [x % p for x in d]
    m, t = 1, n // 2
    while m < n:
        for i in range(m):
            for x in range(2 * i * t, 2 * i * t + t):
                u, v = a[x], a[x + t] * fw[m + i] % p
                a[x], a[x + t] = (u + v) % p, (u - v) % p
        m, t = 2 * m, t // 2
    return a, br


# ---- tests -------------------------------------------------------------------------------------------------------------------

CASES = [((16, Q29, 97, 19), 4), ((16, Q60, 97, 19), 4), ((16, Q60, 97, 19), 16)]
STEPS = [(0, False), (3, False), (0, True), (5, True)]   # g = 1, a rotation, the row swap, a swapped rotation


def setup(params, w):
    n, t = params[0], params[2]
    s, pk0, pk1 = ref_keygen_share(params, b"\x71" * 32, b"\x71" * 32)
    rng = random.Random(n + w)
    v = np.array([rng.randrange(t) for _ in range(n)], dtype=np.uint64)
    m = encode(params, v)
    c0, c1 = ref_encrypt(params, pk0, pk1, m, b"\x72" * 32, 0)
    elements = [galois_element(n, k, swap) for k, swap in STEPS]
    keys = [ref_galois_key(params, s, b"\x73" * 32, b"\x73" * 32, g, w) for g in elements]
    return s, v, m, c0, c1, elements, np.array([k[0] for k in keys]), np.array([k[1] for k in keys])


@pytest.mark.parametrize("params,w", CASES)
def test_hoisted_rotation_decrypts_to_sigma_and_differs_from_apply_galois(params, w):
    n, q, t = params[0], params[1], params[2]
    s, v, m, c0, c1, elements, gk0, gk1 = setup(params, w)
    assert elements[0] == 1 and elements[2] == 2 * n - 1
    differs = 0
    for k, g in enumerate(elements):
        r0, r1 = ref_hoisted_rotation(params, c0, c1, g, gk0[k], gk1[k], w)
        want = sigma(m, g, q)
        assert np.array_equal(ref_decrypt(params, s, r0, r1)[0], want), g
        assert np.array_equal(eval_slots(params, want), rotate(v, *STEPS[k])), g
        o0, o1 = ref_apply_galois(params, c0, c1, g, gk0[k], gk1[k], w)
        assert np.array_equal(ref_decrypt(params, s, o0, o1)[0], want), g
        hoisted, plain = ref_noise(params, s, r0, r1, want), ref_noise(params, s, o0, o1, want)
        print("g = %d: noise 2^%.1f hoisted, 2^%.1f apply_galois" % (g, np.log2(max(hoisted, 1)), np.log2(max(plain, 1))))
        if g == 1:
            assert np.array_equal(r0, c0) and np.array_equal(r1, c1)
        else:
            differs += not (np.array_equal(r0, o0) and np.array_equal(r1, o1))
            assert hoisted < 8 * max(plain, 1) and plain < 8 * max(hoisted, 1)   # the same noise size
    assert differs >= 1


@pytest.mark.parametrize("params,w", CASES)
def test_linear_transform_decrypts_to_the_slot_formula(params, w):
    n, q, t = params[0], params[1], params[2]
    s, v, m, c0, c1, elements, gk0, gk1 = setup(params, w)
    rng = random.Random(7 * w)
    d = np.array([[rng.randrange(t) for _ in range(n)] for _ in elements], dtype=np.uint64)
    diag = np.array([encode(params, dk) for dk in d])
    o0, o1 = ref_linear_transform(params, c0, c1, elements, gk0, gk1, w, diag)
    got = ref_decrypt(params, s, o0, o1)[0]
    want = transform_slots(params, v, STEPS, d)
    noise = ref_noise(params, s, o0, o1, got)
    print("noise 2^%.1f of 2^%.1f" % (np.log2(max(noise, 1)), np.log2(q // t // 2)))
    assert np.array_equal(eval_slots(params, got), want)
    # the same thing through the ring: sum_k sigma_g(m) p_k mod T
    acc = kron_negacyclic([(centred(deg(sigma(m, g, q)), q), centred(deg(p), q)) for g, p in zip(elements, diag)], n)
    assert np.array_equal(got, circ([(x + t // 2) % t - t // 2 for x in acc], q))


def test_linear_transform_is_the_sum_of_plain_products():
    """bit for bit zkfhe_bfv_mul_plain of every hoisted rotation (centred lifts, exact product, mod Q), summed with zkfhe_bfv_add"""
    params, w = (16, Q60, 97, 19), 16
    n, q = params[0], params[1]
    s, v, m, c0, c1, elements, gk0, gk1 = setup(params, w)
    diag = np.array([encode(params, [(3 * k + p) % 97 for p in range(n)]) for k in range(len(elements))])
    o = ref_linear_transform(params, c0, c1, elements, gk0, gk1, w, diag)
    acc = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
    for k, g in enumerate(elements):
        r = ref_hoisted_rotation(params, c0, c1, g, gk0[k], gk1[k], w)
        for j in (0, 1):
            prod = circ(kron_negacyclic([(centred(deg(r[j]), q), centred(deg(diag[k]), q))], n), q)
            acc[j] = np.array([(int(a) + int(b)) % q for a, b in zip(acc[j], prod)], dtype=np.uint64)
    assert np.array_equal(o[0], acc[0]) and np.array_equal(o[1], acc[1])


@pytest.mark.parametrize("n,p", [(16, 97), (64, 12289)])
def test_ntt_domain_index_rule(n, p):
    """the transform of sigma_g(d) at index k is the transform of d at the index k' with 2 br(k') + 1 = (2 br(k) + 1) g mod 2N"""
    log_n = n.bit_length() - 1
    r = next(x for x in range(2, p) if pow(x, (p - 1) // 2, p) != 1 and all(pow(x, (p - 1) // f, p) != 1 for f in (2, 3)))
    psi = pow(r, (p - 1) // (2 * n), p)
    assert pow(psi, n, p) == p - 1
    rng = random.Random(n)
    d = [rng.randrange(-50, 50) for _ in range(n)]
    hat, br = small_ntt(d, n, p, psi)
    for k in range(n):   # index k holds the evaluation at psi^(2 br(k) + 1)
        e = 2 * br(k, log_n) + 1
        assert hat[k] == sum(x * pow(psi, e * i, p) for i, x in enumerate(d)) % p
    for g in (1, 3, 5, 2 * n - 1, 5 * (2 * n - 1) % (2 * n), pow(5, 3, 2 * n)):
        rot, _ = small_ntt(sigma_z(d, g), n, p, psi)
        for k in range(n):
            e = (2 * br(k, log_n) + 1) * g % (2 * n)
            assert rot[k] == hat[br((e - 1) // 2, log_n)], (g, k)
        # neighbouring indices stay inside one aligned block: the gather of 64 (here 4) indices is a permutation of a block
        blk = 4
        for base in range(0, n, blk):
            src = {br(((2 * br(k, log_n) + 1) * g % (2 * n) - 1) // 2, log_n) // blk for k in range(base, base + blk)}
            assert len(src) == 1


@pytest.mark.parametrize("n,t", [(16, 97), (64, 257)])
def test_matrix_diagonals_reproduce_the_product(n, t):
    params = (n, Q60, t, 19)
    rng = np.random.default_rng(n)
    dense = rng.integers(0, t, size=(n, n), dtype=np.uint64)
    band = np.zeros((n, n), dtype=np.uint64)
    for p in range(n):   # a band inside each row block, and one entry across the rows
        for off in (0, 1, 3):
            band[p, (p // (n // 2)) * (n // 2) + (p + off) % (n // 2)] = rng.integers(1, t)
    band[2, n // 2 + 2] = 5
    for matrix, count in ((dense, n), (band, 4)):
        v = rng.integers(0, t, size=n, dtype=np.uint64)
        elements, d = zk.bfv_matrix_diagonals(params, matrix)
        assert len(elements) == count == d.shape[0] and d.shape[1] == n
        acc = np.zeros(n, dtype=object)
        for g, dk in zip(elements, d):
            steps, swap = next((k, sw) for sw in (False, True) for k in range(n // 2) if galois_element(n, k, sw) == g)
            acc = (acc + dk.astype(object) * rotate(v, steps, swap).astype(object)) % t
        assert np.array_equal(acc.astype(np.uint64), (matrix.astype(object) @ v.astype(object) % t).astype(np.uint64))
    elements, d = zk.bfv_matrix_diagonals(params, np.zeros((n, n), dtype=np.int64))
    assert elements == [] and d.shape == (0, n)
    elements, d = zk.bfv_matrix_diagonals(params, -np.eye(n, dtype=np.int64))
    assert elements == [1] and np.array_equal(d[0], np.full(n, t - 1, dtype=np.uint64))
    with pytest.raises(ValueError):
        zk.bfv_matrix_diagonals(params, np.zeros((n, n + 1)))
    with pytest.raises(zk.ZkfheError, match="batching"):
        zk.bfv_matrix_diagonals((n, Q60, 7, 19), np.zeros((n, n)))


def test_new_symbols_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    for name in METHODS:
        assert callable(getattr(zk.Context, name)), name
    assert callable(zk.bfv_matrix_diagonals)
    assert zk.PROF_BFV_HOIST == 16 and zk.PROF_BFV_LINEAR == 17
    assert re.search(r"#define ZKFHE_PROF_BFV_HOIST 16\b", header) and re.search(r"#define ZKFHE_PROF_BFV_LINEAR 17\b", header)
    for word in ("NOT from", "> 150", "element-major", "neither read nor checked"):
        assert word in header, word
