"""Host side of the rotation edge tests (no GPU): the input generators that tests/test_gpu_bfv_rotation_edges.py runs, checked against
the restatements of the sibling host files.  The range rule of zkfhe_bfv_linear_transform restated, with its bit counts on both sides
of the 150 / 151 boundary; worst-case inputs whose exact sum before the reduction mod Q reaches 2^145 in both signs; the
recomposition key of the digit-width sweep against its closed form; the element lists of the small rings and of the tile sweep; and
every generator inside the documented input ranges."""
import functools

import numpy as np
import pytest

from tests.test_bfv_bsgs_host import bsgs_slots, ref_linear_transform_bsgs, steps_of
from tests.test_bfv_edges_host import Q62, QE
from tests.test_bfv_eval_host import Q29, Q60, Q63, centred, circ, deg, kron_negacyclic, relin_digits
from tests.test_bfv_galois_host import (batching, encode, eval_slots, galois_element, ref_apply_galois, ref_galois_key, rotate, sigma)
from tests.test_bfv_linear_host import ref_hoisted_rotation, ref_linear_transform, sigma_z, transform_slots
from tests.test_bfv_threshold_host import ref_decrypt, ref_encrypt, ref_keygen_share

# the small rings: (N, T), every T a batching modulus; (8, 17) has 2N = T - 1 and 2048 is the largest ring that 12289 batches
RINGS = [(8, 17), (16, 97), (64, 257), (512, 12289), (2048, 12289)]
SWEEP = (16, Q60, 97, 19)            # the tile sweep, w = 16
MANY = (64, Q60, 257, 19)            # 600 elements, w = 32
EDGE = (8, Q63, Q63 - 2, 19)         # the range rule's boundary
# (params, w, elements): the rule gives 150 bits at each, and the exact sum reaches 2^145
WORST = [(EDGE, 14, [3]), (EDGE, 14, [15]), ((16, Q63, Q63 - 2, 19), 12, [5]), (EDGE, 13, [3, 15, 5])]


# ---- the range rule, restated from zkfhe.h -------------------------------------------------------------------------------------

def range_bits(params, n_elems, w):
    """bitlen(n_elems) + bitlen(N) + bitlen(floor(T/2)) + bitlen(Q - 1) + bitlen(1 + l N (2^w - 1)): refused above 150"""
    n, q, t = params[0], params[1], params[2]
    ks = 1 + relin_digits(q, w) * n * ((1 << w) - 1)
    return n_elems.bit_length() + n.bit_length() + (t // 2).bit_length() + (q - 1).bit_length() + ks.bit_length()


# ---- generators ------------------------------------------------------------------------------------------------------------------

def residues(rng, params, count):
    return rng.integers(0, params[1], size=(count, params[0]), dtype=np.uint64)


def plaintexts(rng, params, shape, ends=True):
    """random plaintexts over the whole range [0, T/2] and [Q - T/2, Q - 1]; with `ends`, the first two coefficients of each are
    floor(T/2) and -floor(T/2)"""
    q, t = params[1], params[2]
    x = rng.integers(-(t // 2), t // 2 + 1, size=tuple(shape) + (params[0],)).astype(object)
    if ends:
        x[..., 0], x[..., 1] = t // 2, -(t // 2)
    return (x % q).astype(np.uint64)


def nonzero_plaintexts(rng, params, shape):
    """as plaintexts, with no zero coefficient (T >= 3)"""
    q, t = params[1], params[2]
    x = rng.integers(1, t // 2 + 1, size=tuple(shape) + (params[0],)).astype(object)
    x = x * rng.choice(np.array([-1, 1], dtype=object), size=x.shape)
    return (x % q).astype(np.uint64)


def random_keys(rng, params, count, w):
    """`count` keys of uniform residues, (gk0, gk1) of shape (count, l, N)"""
    l = relin_digits(params[1], w)
    return tuple(rng.integers(0, params[1], size=(count, l, params[0]), dtype=np.uint64) for _ in range(2))


def ring_steps(n):
    """(steps, swap) of the element list of a small ring: all eight odd g below 16 at N = 8; elsewhere g = 1, two rotations, the
    row swap 2N - 1 and a swapped rotation"""
    if n == 8:
        return [(k, sw) for sw in (False, True) for k in range(4)]
    return [(0, False), (1, False), (n // 2 - 3, False), (0, True), (5 % (n // 2), True)]


def ring_elements(n):
    return [galois_element(n, k, sw) for k, sw in ring_steps(n)]


def split(elements, n_baby):
    """a flat list as baby x giant: the first n_baby entries, and the rest"""
    return list(elements[:n_baby]), list(elements[n_baby:])


def ring_width(n):
    """the digit width of the small-ring tests: narrow enough at the larger rings that a transform of five elements decrypts"""
    return 16 if n <= 64 else 12


def sweep_lists(n_baby, n_giant):
    """the element lists of the tile sweep at N = 16: prefixes of a baby list of 3 and a giant list of 9 with repeats, the row swap
    and g = 1 in both (a list of one element holds a rotation)"""
    n = SWEEP[0]
    baby = [galois_element(n, 1), 1, galois_element(n, 2, True)]
    giant = [galois_element(n, 3), 1, 2 * n - 1, galois_element(n, 3), galois_element(n, 6, True), 1, galois_element(n, 5), 2 * n - 1,
             galois_element(n, 7)]
    return baby[:n_baby], giant[:n_giant]


def many_elements(count):
    """`count` elements cycling through all 64 odd g below 2N = 128 (g = 1 among them)"""
    return [(2 * k + 1) % (2 * MANY[0]) for k in range(count)]


def const_poly(n, v, q):
    """the constant polynomial v (degree 0 sits at position N - 1 in CircuitInput order)"""
    p = np.zeros(n, dtype=np.uint64)
    p[n - 1] = int(v) % q
    return p


def recomposition_key(n, q, w):
    """gk0_i = the constant 2^(i w) mod Q, gk1_i = 0: sum_i D_i 2^(i w) = the polynomial the digits were taken of"""
    l = relin_digits(q, w)
    return np.stack([const_poly(n, pow(2, i * w, q), q) for i in range(l)]), np.zeros((l, n), dtype=np.uint64)


def width_values(q, w):
    """the c1 coefficients of the width sweep: 0, 1, Q - 1, 2^w - 1, 2^w, and 2^(k w) - 1, 2^(k w), (2^w - 1) << ((k - 1) w) for
    every k where the value is below Q; distinct, in this order"""
    l = relin_digits(q, w)
    vs = [0, 1, q - 1, (1 << w) - 1, 1 << w]
    for k in range(1, l + 1):
        vs += [(1 << (k * w)) - 1, 1 << (k * w), ((1 << w) - 1) << ((k - 1) * w)]
    out = []
    for v in vs:
        if v < q and v not in out:
            out.append(v)
    return out


def width_rows(rng, n, q, w):
    """the values of width_values as rows of N coefficients (CircuitInput order), the last row padded with random residues"""
    vs = width_values(q, w)
    vs += [int(x) for x in rng.integers(0, q, size=-len(vs) % n, dtype=np.uint64)]
    return np.array([circ(vs[i:i + n], q) for i in range(0, len(vs), n)], dtype=np.uint64)


def sigma_sum(c0, c1, g, q):
    """sigma_g(c0) + sigma_g(c1) mod Q: what the recomposition key makes of a rotation"""
    return np.array([(int(a) + int(b)) % q for a, b in zip(sigma(c0, g, q), sigma(c1, g, q))], dtype=np.uint64)


# ---- the exact sum of zkfhe_bfv_linear_transform before its reduction mod Q ------------------------------------------------------

def exact_rotation(params, c0, c1, g, gk0, gk1, w):
    """the hoisted rotation as the integers the definition sums before any reduction: c0 read centred, the digits and the key words as
    non-negative integers; degree order"""
    n, q = params[0], params[1]
    if g == 1:
        return centred(deg(c0), q), deg(c1)
    l, d1 = relin_digits(q, w), deg(c1)
    digits = [sigma_z([(c >> (i * w)) & ((1 << w) - 1) for c in d1], g) for i in range(l)]
    k0 = kron_negacyclic([(digits[i], deg(gk0[i])) for i in range(l)], n)
    k1 = kron_negacyclic([(digits[i], deg(gk1[i])) for i in range(l)], n)
    return [x + y for x, y in zip(sigma_z(centred(deg(c0), q), g), k0)], k1


def exact_transform(params, c0, c1, elements, gk0, gk1, w, diag):
    """sum_k r_k p_k over Z with r_k of exact_rotation and p_k the centred diagonal: two lists of signed integers in degree order,
    congruent mod Q to ref_linear_transform"""
    n, q = params[0], params[1]
    rot = [exact_rotation(params, c0, c1, g, gk0[k], gk1[k], w) for k, g in enumerate(elements)]
    p = [centred(deg(d), q) for d in diag]
    return tuple(kron_negacyclic([(r[j], pk) for r, pk in zip(rot, p)], n) for j in (0, 1))


@functools.lru_cache(maxsize=None)
def best_support(n, g):
    """the support pattern (a tuple of 0 / 1 in degree order) of a key row over {0, Q - 1} that maximises sum_k |r[k]| for
    r = sigma_g(constant digits) times the row: exhaustive over the 2^N - 1 non-empty patterns"""
    s = sigma_z([1] * n, g)
    m = np.zeros((n, n), dtype=np.int64)   # r = m @ pattern: the negacyclic product with the sign vector of sigma_g
    for i in range(n):
        for j in range(n):
            m[(i + j) % n, j] += s[i] if i + j < n else -s[i]
    patterns = (np.arange(1, 1 << n, dtype=np.int64)[:, None] >> np.arange(n)) & 1
    score = np.abs(patterns @ m.T).sum(axis=1)
    return tuple(int(b) for b in patterns[int(score.argmax())])


def worst_case(params, w, elements):
    """Inputs that drive the accepted side of the range rule: c1 with every coefficient 2^62 - 1 (every digit below the top bit all
    ones), both key rows of every digit of element k on the support best_support(N, g_k) over {0, Q - 1}, c0 = +-floor(Q/2) with
    the signs of the first element's key products, and diagonals +-floor(T/2) signed so that every term of output coefficient N - 1
    has the same sign.  Returns c0, c1 (one ciphertext), gk0, gk1 and the diagonals; the negated diagonals give the other sign."""
    n, q, t = params[0], params[1], params[2]
    l = relin_digits(q, w)
    c1 = np.full(n, (1 << 62) - 1, dtype=np.uint64)
    gk0 = np.zeros((len(elements), l, n), dtype=np.uint64)
    for k, g in enumerate(elements):
        gk0[k, :] = circ([b * (q - 1) for b in best_support(n, g)], q)
    gk1 = gk0.copy()
    zero = np.zeros(n, dtype=np.uint64)
    r = exact_rotation(params, zero, c1, elements[0], gk0[0], gk1[0], w)[1]
    want = [q // 2 if x >= 0 else -(q // 2) for x in r]              # sigma_g(c0), in the signs of the key products
    c0 = circ(sigma_z(want, pow(elements[0], -1, 2 * n)), q)
    diag = []
    for k, g in enumerate(elements):
        r = exact_rotation(params, c0, c1, g, gk0[k], gk1[k], w)[1]
        p = [0] * n
        for j, x in enumerate(r):   # coefficient N - 1 of r p is sum_j r[j] p[N - 1 - j], with no wrap
            p[n - 1 - j] = t // 2 if x >= 0 else -(t // 2)
        diag.append(circ(p, q))
    return c0, c1, gk0, gk1, np.array(diag)


def negated(params, diag):
    q = params[1]
    return np.array([[(q - int(x)) % q for x in row] for row in diag], dtype=np.uint64)


# ---- what the documented input ranges are ---------------------------------------------------------------------------------------

def in_ranges(params, cts=(), keys=(), diags=(), elements=(), slots=()):
    """ciphertexts and keys below Q, diagonals in [0, T/2] or [Q - T/2, Q - 1], elements odd and below 2N, slot values below T"""
    n, q, t = params[0], params[1], params[2]
    ok = all(np.asarray(a).dtype == np.uint64 and np.asarray(a).shape[-1] == n and int(np.asarray(a).max()) < q for a in list(cts) + list(keys))
    for d in diags:
        d = np.asarray(d)
        ok = ok and d.dtype == np.uint64 and bool(np.all((d <= t // 2) | ((d >= q - t // 2) & (d < q))))
    ok = ok and all(g % 2 == 1 and 0 < g < 2 * n for g in elements)
    return ok and all(int(np.asarray(v).max()) < t for v in slots)


# ---- tests -----------------------------------------------------------------------------------------------------------------------

def test_range_rule_bit_counts():
    assert (range_bits(EDGE, 1, 14), range_bits(EDGE, 1, 15)) == (150, 151)
    assert (range_bits(EDGE, 3, 13), range_bits(EDGE, 3, 14)) == (150, 151)
    for params, w, elements in WORST:
        assert range_bits(params, len(elements), w) == 150
    # the many-element case, as 10 + 7 + 8 + 60 + 39 and 6 + 7 + 8 + 60 + 39
    assert 1 + 2 * 64 * ((1 << 32) - 1) < 1 << 39 and relin_digits(Q60, 32) == 2
    assert range_bits(MANY, 600, 32) == 124 and range_bits(MANY, 40, 32) == 120
    assert 600 << 62 > 1 << 64   # a sum over the elements carried unreduced in 64 bits would overflow
    # T at its ends at N = 8, w = 4
    assert range_bits((8, Q60, Q60 - 2, 19), 1, 4) == 135 and range_bits((8, Q60, 2, 19), 4, 4) <= 150
    assert range_bits((8, Q60, Q60 - 2, 19), 4, 4) <= 150
    # the refusal the sibling files test, far from the boundary: 1 + 16 + 30 + 63 + 48
    assert range_bits((32768, Q63, 2013265921, 19), 1, 32) == 158
    # every other accepted call of the GPU file
    for n, t in RINGS:
        assert range_bits((n, Q60, t, 19), len(ring_elements(n)), ring_width(n)) <= 150
    assert range_bits(SWEEP, 5, 16) <= 150
    for q in (Q63, Q62):
        for w in (1, 7, 13, 21, 31, 32):
            assert range_bits((64, q, 65537, 19), 3, w) <= 150, (q, w)
    assert range_bits((64, Q29, 65537, 19), 3, 32) <= 150
    for params, ws in (((8, 3, 2, 1), (1, 2, 32)), ((16, Q62, 1 << 20, 19), (31,)), ((16, QE, 97, 19), (7,))):
        for w in ws:
            assert range_bits(params, 3, w) <= 150


def test_digit_counts_where_l_w_is_the_bit_length():
    assert relin_digits(Q63, 21) * 21 == 63 == (Q63 - 1).bit_length()
    assert relin_digits(Q62, 31) * 31 == 62 == (Q62 - 1).bit_length()
    assert relin_digits(Q29, 29) == 1 == relin_digits(Q29, 32) and (Q29 - 1).bit_length() == 29
    assert relin_digits(Q60, 32) == 2 and relin_digits(3, 1) == 2 and relin_digits(3, 2) == 1


@pytest.mark.parametrize("params,w,elements", WORST)
def test_worst_case_inputs_reach_2_145_in_both_signs(params, w, elements):
    n, q, t = params[0], params[1], params[2]
    c0, c1, gk0, gk1, diag = worst_case(params, w, elements)
    assert in_ranges(params, cts=[c0, c1], keys=[gk0, gk1], diags=[diag, negated(params, diag)], elements=elements)
    assert all(g != 1 for g in elements)
    assert set(int(x) for x in c1) == {(1 << 62) - 1}
    assert set(int(x) for x in c0) <= {q // 2, q - q // 2} and set(int(x) for x in diag.reshape(-1)) <= {t // 2, q - t // 2}
    l = relin_digits(q, w)
    digits = [(((1 << 62) - 1) >> (i * w)) & ((1 << w) - 1) for i in range(l)]
    assert all(d == (1 << w) - 1 for d in digits[:-1]) and digits[-1] == (1 << (62 - (l - 1) * w)) - 1
    limit = 1 << 150   # what the rule allows the sum to reach
    reached = []
    for d in (diag, negated(params, diag)):
        exact = exact_transform(params, c0, c1, elements, gk0, gk1, w, d)
        want = ref_linear_transform(params, c0, c1, elements, gk0, gk1, w, d)
        for j in (0, 1):
            assert np.array_equal(circ(exact[j], q), want[j])
            assert max(abs(x) for x in exact[j]) < limit
        reached.append([exact[j][n - 1] for j in (0, 1)])
    print("N = %d, w = %d, elements %s: |exact sum| reaches 2^%.1f" % (n, w, elements, np.log2(float(abs(reached[0][0])))))
    for j in (0, 1):
        assert reached[0][j] >= 1 << 145 and reached[1][j] <= -(1 << 145), j


def test_best_support_is_the_maximum():
    """the search against a schoolbook negacyclic product over every pattern at N = 8"""
    n = 8
    for g in (3, 15):
        s = sigma_z([1] * n, g)
        best = 0
        for mask in range(1, 1 << n):
            pat = [(mask >> i) & 1 for i in range(n)]
            best = max(best, sum(abs(x) for x in kron_negacyclic([(s, pat)], n)))
        assert sum(abs(x) for x in kron_negacyclic([(s, list(best_support(n, g)))], n)) == best


def test_generators_stay_inside_the_documented_ranges():
    rng = np.random.default_rng(1)
    for n, t in RINGS[:3]:
        params = (n, Q60, t, 19)
        g = ring_elements(n)
        keys = random_keys(rng, params, len(g), ring_width(n))
        assert keys[0].shape == (len(g), relin_digits(Q60, ring_width(n)), n)
        assert in_ranges(params, cts=[residues(rng, params, 3)], keys=keys, diags=[plaintexts(rng, params, (len(g),))], elements=g)
    for params in ((8, Q60, 2, 19), (8, Q60, Q60 - 2, 19), (8, 3, 2, 1), (16, Q62, 1 << 20, 19), (16, QE, 97, 19), MANY, SWEEP):
        q, t = params[1], params[2]
        d = plaintexts(rng, params, (2, 3))
        assert in_ranges(params, cts=[residues(rng, params, 2)], keys=random_keys(rng, params, 2, 4), diags=[d])
        assert np.all(d[..., 0] == t // 2) and np.all(d[..., 1] == q - t // 2)
    d = nonzero_plaintexts(rng, SWEEP, (9, 3))
    assert in_ranges(SWEEP, diags=[d]) and d.all()
    for nb in (1, 3):
        for ng in (1, 3, 4, 5, 7, 8, 9):
            baby, giant = sweep_lists(nb, ng)
            assert len(baby) == nb and len(giant) == ng and in_ranges(SWEEP, elements=baby + giant)
    baby, giant = sweep_lists(3, 9)
    assert 1 in baby and 1 in giant and len(set(giant)) < len(giant)
    g = many_elements(600)
    assert in_ranges(MANY, elements=g) and set(g) == set(range(1, 128, 2)) and g.count(1) >= 9
    for q in (Q63, Q62, QE, Q29, 3):
        for w in range(1, 33):
            params = (64, q, 2, 1)
            rows = width_rows(rng, 64, q, w)
            l = relin_digits(q, w)
            assert in_ranges(params, cts=[rows], keys=recomposition_key(64, q, w))
            assert any(int(x) >> ((l - 1) * w) for x in rows.reshape(-1))   # the top digit is used
            assert set(width_values(q, w)) <= set(int(x) for x in rows.reshape(-1))
            assert {0, 1 % q, q - 1} <= set(width_values(q, w)) and all(v < q for v in width_values(q, w))


def test_ring_elements_cover_the_small_rings():
    assert sorted(ring_elements(8)) == list(range(1, 16, 2))
    for n, t in RINGS:
        assert batching(n, t)
        g = ring_elements(n)
        assert g[0] == 1 and 2 * n - 1 in g and len(set(g)) == len(g) and in_ranges((n, Q60, t, 19), elements=g)
        assert [steps_of(n, x) for x in g] == ring_steps(n) or n > 64   # steps_of is a linear search
    assert RINGS[0][1] - 1 == 2 * RINGS[0][0] and not batching(4096, 12289)


@pytest.mark.parametrize("n,t", RINGS[:2])
def test_small_ring_transforms_decrypt_to_the_slot_formulas(n, t):
    """the restatements at the smallest rings, with the keys of the restated key generation: rotations, the flat transform and its
    baby x giant split decrypt to rotate, transform_slots and bsgs_slots"""
    params, w = (n, Q60, t, 19), ring_width(n)
    q = params[1]
    rng = np.random.default_rng(n)
    s, pk0, pk1 = ref_keygen_share(params, b"\x61" * 32, b"\x61" * 32)
    v = rng.integers(0, t, size=n, dtype=np.uint64)
    v[0], v[1] = 0, t - 1
    m = encode(params, v)
    assert np.array_equal(eval_slots(params, m), v)
    c0, c1 = ref_encrypt(params, pk0, pk1, m, b"\x62" * 32, 0)
    steps, elements = ring_steps(n), ring_elements(n)
    keys = [ref_galois_key(params, s, b"\x63" * 32, b"\x63" * 32, g, w) for g in elements]
    gk0, gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    for k, g in enumerate(elements):
        r0, r1 = ref_hoisted_rotation(params, c0, c1, g, gk0[k], gk1[k], w)
        assert np.array_equal(eval_slots(params, ref_decrypt(params, s, r0, r1)[0]), rotate(v, *steps[k])), g
    d = rng.integers(0, t, size=(len(elements), n), dtype=np.uint64)
    o0, o1 = ref_linear_transform(params, c0, c1, elements, gk0, gk1, w, np.array([encode(params, dk) for dk in d]))
    assert np.array_equal(eval_slots(params, ref_decrypt(params, s, o0, o1)[0]), transform_slots(params, v, steps, d))
    nb = 3 if n == 8 else 2
    (gb, gg), (sb, sg) = split(elements, nb), split(steps, nb)
    d = rng.integers(0, t, size=(len(gg), nb, n), dtype=np.uint64)
    diag = np.array([[encode(params, x) for x in row] for row in d])
    o0, o1 = ref_linear_transform_bsgs(params, c0, c1, gb, gk0[:nb], gk1[:nb], gg, gk0[nb:], gk1[nb:], w, diag)
    assert np.array_equal(eval_slots(params, ref_decrypt(params, s, o0, o1)[0]), bsgs_slots(params, v, sb, sg, d))


@pytest.mark.parametrize("q", [Q63, Q62, QE])
def test_recomposition_key_gives_sigma_of_the_sum(q):
    """with gk0_i = 2^(i w) and gk1_i = 0 both restated rotations are (sigma_g(c0) + sigma_g(c1), 0), whatever the width"""
    n = 64
    params = (n, q, 65537, 19)
    rng = np.random.default_rng(q % 1013)
    for w in (1, 7, 21, 31, 32):
        gk0, gk1 = recomposition_key(n, q, w)
        c1 = width_rows(rng, n, q, w)[0]
        c0 = residues(rng, params, 1)[0]
        for g in (3, 2 * n - 1):
            want = sigma_sum(c0, c1, g, q)
            for ref in (ref_apply_galois, ref_hoisted_rotation):
                o0, o1 = ref(params, c0, c1, g, gk0, gk1, w)
                assert np.array_equal(o0, want) and not o1.any(), (w, g)
