"""Edges of GPU BFV (bfv_enc.hip, bfv_eval.hip, rns_ntt.hip.hpp) that test_gpu_bfv_encrypt.py and test_gpu_bfv_eval.py do not
reach: batches that cross the chunk boundary of every batched call, rounding at exact ties (even Q), relinearization digits of
every width, and parameter corners (rings down to N = 8, Q = 3, T = 2, T near Q/2 and Q, B = 1023, the mul_plain CRT bound).
Every expectation is restated on Python integers from the definitions in zkfhe.h, with the oracles of the host test files.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from tests.test_bfv_edges_host import Q62, TIE_PARAMS, decrypt_value, round_q, tie_values
from tests.test_bfv_eval_host import Q60, Q63, centred, circ, deg, kron_negacyclic, ref_mul, ref_tensor, relin_digits
from tests.test_gpu_bfv_encrypt import error, negacyclic, random_m, ternary, uniform
from tests.test_gpu_bfv_eval import host_noise, plain_product

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


# ---- helpers -----------------------------------------------------------------------------------------------------------------

def chunk_polys(n):
    """polynomials per chunk of every batched call (rns_ntt.hip.hpp): 2^21 coefficients, at least 8 polynomials"""
    return max(8, (1 << 21) // n)


def boundary_rows(count, chunk):
    """the first row, both sides of the first chunk boundary, and the last row"""
    assert chunk < count
    return sorted({0, chunk - 1, chunk, count - 1})


def residues(rng, shape, q):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def const_poly(n, v, q):
    """the constant polynomial v (degree 0 sits at position N - 1 in CircuitInput order)"""
    p = np.zeros(n, dtype=np.uint64)
    p[n - 1] = int(v) % q
    return p


def obj(x):
    return np.asarray(x, dtype=np.uint64).astype(object)


def centred_obj(x, q):
    """residues of any shape -> centred Python integers, same shape"""
    x = obj(x)
    return np.where(x > q // 2, x - q, x)


def samples(values, n, rng, q):
    """`values` (signed, degree order, duplicates by residue dropped) padded with random centred values to N coefficients"""
    seen, out = set(), []
    for v in values:
        if int(v) % q not in seen:
            seen.add(int(v) % q)
            out.append(int(v))
    assert len(out) <= n, (len(out), n)
    return out + [int(rng.integers(0, q)) - q // 2 for _ in range(n - len(out))]


def c1_times_s(c1, sk, q):
    return negacyclic(c1, sk, q).astype(object)


def restate_relin_key(params, sk, seed, w, rlk0, rlk1):
    """rlk1_i = uniform(seed, 7, i); rlk0_i = 2^(i w) s^2 - rlk1_i s - error(seed, 8, i) mod Q (zkfhe.h)"""
    n, q, b = params[0], params[1], params[3]
    l = relin_digits(q, w)
    assert rlk0.shape == rlk1.shape == (l, n)
    s2 = circ(kron_negacyclic([(centred(deg(sk), q), centred(deg(sk), q))], n), q).astype(object)
    for i in range(l):
        a = uniform(seed, 7, i, n, q)
        assert np.array_equal(rlk1[i], a), i
        want = (s2 * pow(2, i * w, q) - c1_times_s(a, sk, q) - obj(error(seed, 8, i, n, q, b))) % q
        assert np.array_equal(obj(rlk0[i]), want), i


def restate_keypair_and_encryption(ctx, params, kseed, eseed, m, first=0):
    """every sample of bfv_fhe_keypair and bfv_encrypt restated from ChaCha20, and the ciphertext formula"""
    n, q, t, b = params
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, kseed)
    assert np.array_equal(sk, ternary(kseed, 4, 0, n, q))
    assert np.array_equal(pk1, uniform(kseed, 5, 0, n, q))
    e = obj(error(kseed, 6, 0, n, q, b))
    assert np.array_equal(obj(pk0), (-(c1_times_s(pk1, sk, q) + e)) % q)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, eseed, first_index=first)
    delta = q // t
    for j in range(m.shape[0]):
        u = ternary(eseed, 1, first + j, n, q)
        e0, e1 = error(eseed, 2, first + j, n, q, b), error(eseed, 3, first + j, n, q, b)
        assert np.array_equal(ct["u"][j], u) and np.array_equal(ct["e0"][j], e0) and np.array_equal(ct["e1"][j], e1), j
        assert np.abs(centred_obj(e0, q)).max() <= b and np.abs(centred_obj(e1, q)).max() <= b
        assert np.array_equal(obj(ct["c0"][j]), (c1_times_s(pk0, u, q) + obj(m[j]) * delta + obj(e0)) % q), j
        assert np.array_equal(obj(ct["c1"][j]), (c1_times_s(pk1, u, q) + obj(e1)) % q), j
    return sk, pk0, pk1, ct


def decrypt_formula(params, sk, c0, c1):
    """inputs.decrypt restated on Python integers for one ciphertext: round(T [c0 + c1 s]_Q / Q) mod T as residues mod Q"""
    q, t = params[1], params[2]
    v = (obj(c0) + c1_times_s(c1, sk, q)) % q
    return np.array([decrypt_value(x, q, t) for x in v], dtype=np.uint64)


def as_plain(x, params):
    """integers (a sum of centred plaintexts) mod T, centred like the decryption, as residues mod Q"""
    q, t = params[1], params[2]
    x = np.asarray(x, dtype=object) % t
    return np.array([int(v - t) % q if v > t // 2 else int(v) for v in x.reshape(-1)], dtype=np.uint64).reshape(x.shape)


# ---- 1. chunk boundaries -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,count", [(8192, 257), (32768, 65)])
def test_chunks_poly_mul_ternary(ctx, n, count):
    q, chunk = Q63, chunk_polys(n)
    rng = np.random.default_rng(n + count)
    a = residues(rng, (count, n), q)
    s = rng.choice(np.array([0, 1, q - 1], dtype=np.uint64), size=(count, n))
    shared = ctx.poly_mul_ternary_negacyclic(a[0], s, q)   # a_count = 1
    per = ctx.poly_mul_ternary_negacyclic(a, s, q)         # a_count = n_polys
    for j in boundary_rows(count, chunk):   # a one-row call never enters the chunk loop
        assert np.array_equal(per[j], ctx.poly_mul_ternary_negacyclic(a[j], s[j:j + 1], q)[0]), j
        assert np.array_equal(shared[j], ctx.poly_mul_ternary_negacyclic(a[0], s[j:j + 1], q)[0]), j
    for j in (chunk - 1, chunk, count - 1):
        assert np.array_equal(per[j], negacyclic(a[j], s[j], q)), j
        assert np.array_equal(shared[j], negacyclic(a[0], s[j], q)), j


def test_chunks_encrypt_and_decrypt(ctx):
    n, count = 8192, 257
    params = (n, Q60, 65537, 19)
    q, t, b = params[1], params[2], params[3]
    chunk = chunk_polys(n)
    first = (1 << 32) - 100   # the index's low word wraps at row 100
    kseed, eseed = b"\x71" * 32, bytes(range(7, 39))
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, kseed)
    m = random_m(np.random.default_rng(257), (count, n), q, t)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, eseed, first_index=first)
    delta = q // t
    for j in boundary_rows(count, chunk) + [100]:
        u = ternary(eseed, 1, first + j, n, q)
        e0, e1 = error(eseed, 2, first + j, n, q, b), error(eseed, 3, first + j, n, q, b)
        assert np.array_equal(ct["u"][j], u), j
        assert np.array_equal(ct["e0"][j], e0) and np.array_equal(ct["e1"][j], e1), j
        assert np.array_equal(obj(ct["c0"][j]), (c1_times_s(pk0, u, q) + obj(m[j]) * delta + obj(e0)) % q), j
        assert np.array_equal(obj(ct["c1"][j]), (c1_times_s(pk1, u, q) + obj(e1)) % q), j
        one = ctx.bfv_encrypt(params, pk0, pk1, m[j], eseed, first_index=first + j)
        for k in ("u", "e0", "e1", "c0", "c1"):
            assert np.array_equal(one[k][0], ct[k][j]), (j, k)
    for k in ("u", "e0", "e1"):   # no two rows share a draw
        assert len({row.tobytes() for row in ct[k]}) == count, k
    assert np.array_equal(ctx.bfv_decrypt(params, sk, ct["c0"], ct["c1"]), m)


def test_chunks_decrypt_and_noise(ctx):
    # [c0 + c1 s]_Q = delta m + e_j with max |e_j| = R_j, a different bound per row: decryption gives m and the noise R_j exactly
    n, count = 8192, 257
    params = (n, Q60, 65537, 19)
    q, t = params[1], params[2]
    chunk = chunk_polys(n)
    rng = np.random.default_rng(8192)
    sk, _, _ = ctx.bfv_fhe_keypair(params, b"\x72" * 32)
    m = random_m(rng, (count, n), q, t)
    R = [1000 + 37 * j for j in range(count)]
    c0 = np.empty((count, n), dtype=np.uint64)
    c1 = np.zeros((count, n), dtype=np.uint64)
    delta = q // t
    for j in range(count):
        e = rng.integers(-R[j], R[j] + 1, size=n).astype(object)
        e[rng.integers(0, n)] = R[j] if j % 2 else -R[j]
        x = obj(m[j]) * delta + e
        if j in boundary_rows(count, chunk):   # c1 = 0 elsewhere: a row that read another row's c1 would still be caught here
            c1[j] = residues(rng, n, q)
            x = x - c1_times_s(c1[j], sk, q)
        c0[j] = np.array([int(v) % q for v in x], dtype=np.uint64)
    dec = ctx.bfv_decrypt(params, sk, c0, c1)
    assert np.array_equal(dec, m)
    noise = ctx.bfv_noise(params, sk, c0, c1)
    assert [int(v) for v in noise] == R
    for j in boundary_rows(count, chunk):
        assert np.array_equal(ctx.bfv_decrypt(params, sk, c0[j], c1[j])[0], dec[j]), j
        assert int(ctx.bfv_noise(params, sk, c0[j], c1[j])[0]) == R[j], j
    for j in (chunk - 1, chunk):
        assert host_noise(params, sk, c0[j:j + 1], c1[j:j + 1]) == [R[j]], j
    # arbitrary residues across the boundary: the decryption formula and the noise restated
    r0, r1 = residues(rng, (count, n), q), residues(rng, (count, n), q)
    dec = ctx.bfv_decrypt(params, sk, r0, r1)
    noise = ctx.bfv_noise(params, sk, r0, r1)
    for j in (chunk - 1, chunk):
        assert np.array_equal(dec[j], decrypt_formula(params, sk, r0[j], r1[j])), j
        assert [int(noise[j])] == host_noise(params, sk, r0[j:j + 1], r1[j:j + 1]), j


def test_chunks_add_subtract(ctx):
    n, count = 1024, 2049
    params = (n, Q60, 7, 19)
    q, chunk = params[1], chunk_polys(n)
    rng = np.random.default_rng(2049)
    a0, a1, b0, b1 = (residues(rng, (count, n), q) for _ in range(4))
    for subtract in (False, True):
        o0, o1 = ctx.bfv_add(params, a0, a1, b0, b1, subtract=subtract)
        sign = -1 if subtract else 1
        assert np.array_equal(obj(o0), (obj(a0) + sign * obj(b0)) % q), subtract
        assert np.array_equal(obj(o1), (obj(a1) + sign * obj(b1)) % q), subtract
        for j in boundary_rows(count, chunk):
            one = ctx.bfv_add(params, a0[j], a1[j], b0[j], b1[j], subtract=subtract)
            assert np.array_equal(one[0][0], o0[j]) and np.array_equal(one[1][0], o1[j]), (subtract, j)


def test_chunks_sum(ctx):
    # 4100 = 2 chunks of 2048 + 4: the accumulator is reset by the first chunk only
    n, count = 1024, 4100
    params = (n, Q60, 7, 19)
    q, chunk = params[1], chunk_polys(n)
    rng = np.random.default_rng(4100)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x73" * 32)
    m = random_m(rng, (count, n), q, params[2])
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x74" * 32)
    c0, c1 = ct["c0"], ct["c1"]
    C0, C1, M = obj(c0), obj(c1), centred_obj(m, q)
    for rows in (count, chunk + 1, 2 * chunk, chunk):
        s0, s1 = ctx.bfv_sum(params, c0[:rows], c1[:rows])
        assert np.array_equal(obj(s0), C0[:rows].sum(axis=0) % q), rows
        assert np.array_equal(obj(s1), C1[:rows].sum(axis=0) % q), rows
        assert np.array_equal(ctx.bfv_decrypt(params, sk, s0, s1)[0], as_plain(M[:rows].sum(axis=0), params)), rows


@pytest.mark.parametrize("shared", [True, False])
def test_chunks_add_plain(ctx, shared):
    n, count = 1024, 2049
    params = (n, Q60, 65537, 19)
    q, t, chunk = params[1], params[2], chunk_polys(n)
    rng = np.random.default_rng(2049 + shared)
    c0, c1 = residues(rng, (count, n), q), residues(rng, (count, n), q)
    pm = random_m(rng, (1 if shared else count, n), q, t)
    o0, o1 = ctx.bfv_add_plain(params, c0, c1, pm[0] if shared else pm)
    assert np.array_equal(obj(o0), (obj(c0) + centred_obj(pm, q) * (q // t)) % q)
    assert np.array_equal(o1, c1)
    for j in boundary_rows(count, chunk):
        one = ctx.bfv_add_plain(params, c0[j], c1[j], pm[0] if shared else pm[j])
        assert np.array_equal(one[0][0], o0[j]) and np.array_equal(one[1][0], o1[j]), j


@pytest.mark.parametrize("shared", [True, False])
def test_chunks_mul_plain(ctx, shared):
    n, count = 8192, 257
    params = (n, Q60, 65537, 19)
    q, t, chunk = params[1], params[2], chunk_polys(n)
    rng = np.random.default_rng(257 + shared)
    c0, c1 = residues(rng, (count, n), q), residues(rng, (count, n), q)
    pm = random_m(rng, (1 if shared else count, n), q, t)
    o0, o1 = ctx.bfv_mul_plain(params, c0, c1, pm[0] if shared else pm)
    for j in boundary_rows(count, chunk):
        mj = pm[0] if shared else pm[j]
        one = ctx.bfv_mul_plain(params, c0[j], c1[j], mj)
        assert np.array_equal(one[0][0], o0[j]) and np.array_equal(one[1][0], o1[j]), j
        if j in (chunk - 1, chunk):
            mc = centred(deg(mj), q)
            assert np.array_equal(o0[j], circ(kron_negacyclic([(centred(deg(c0[j]), q), mc)], n), q)), j
            assert np.array_equal(o1[j], circ(kron_negacyclic([(centred(deg(c1[j]), q), mc)], n), q)), j


@pytest.mark.parametrize("n,count", [(8192, 257), (32768, 65)])
def test_chunks_mul(ctx, n, count):
    params, w = (n, Q60, 65537, 19), 20
    q, chunk = params[1], chunk_polys(n)
    rng = np.random.default_rng(n + 20)
    l = relin_digits(q, w)
    rlk0, rlk1 = residues(rng, (l, n), q), residues(rng, (l, n), q)
    a0, a1, b0, b1 = (residues(rng, (count, n), q) for _ in range(4))
    o0, o1 = ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    for j in boundary_rows(count, chunk):
        one = ctx.bfv_mul(params, a0[j], a1[j], b0[j], b1[j], rlk0, rlk1, base_bits=w)
        assert np.array_equal(one[0][0], o0[j]) and np.array_equal(one[1][0], o1[j]), j
    if n <= 8192:   # the full oracle costs seconds per row at N = 32768
        for j in (chunk - 1, chunk):
            want0, want1 = ref_mul(params, a0[j], a1[j], b0[j], b1[j], rlk0, rlk1, w)
            assert np.array_equal(o0[j], want0) and np.array_equal(o1[j], want1), j


# ---- 2. rounding at exact ties ---------------------------------------------------------------------------------------------------

def multipliers(q, rng):
    """constants c for b0 = c: 1, -1, small, +-floor(Q/2) and an odd random one, distinct non-zero residues"""
    cs, seen = [], set()
    for c in (1, -1, 3, q // 2, -(q // 2), q // 2 - 1, int(rng.integers(1, q // 2 + 1)) | 1):
        if c % q and c % q not in seen:
            seen.add(c % q)
            cs.append(c)
    return cs


@pytest.mark.parametrize("q,t", TIE_PARAMS)
def test_mul_rounds_at_ties(ctx, q, t):
    # b0 = c (a constant), b1 = 0: x0 = c a0, x1 = c a1, x2 = 0, so out = (c^0, c^1) is the rounding of chosen products
    n, w = 128, 16
    params = (n, q, t, 1)
    rng = np.random.default_rng(q % 100003 + t)
    cs = multipliers(q, rng)
    extras = [0, 1, -1, q // 2, -(q // 2)]
    a0, a1, b0 = [], [], []
    for c in cs:
        vals = samples([a for a, _ in tie_values(q, t, c)] + extras, n, rng, q)
        a0.append(circ(vals, q))
        a1.append(circ(vals[::-1], q))
        b0.append(const_poly(n, c, q))
    a0, a1, b0 = np.array(a0), np.array(a1), np.array(b0)
    b1 = np.zeros_like(a0)
    l = relin_digits(q, w)
    rlk0, rlk1 = residues(rng, (l, n), q), residues(rng, (l, n), q)   # c^2 = 0: the key adds nothing
    o0, o1 = ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    exact_ties = 0
    for j, c in enumerate(cs):
        cc = centred([c % q], q)[0]
        for out, a in ((o0[j], a0[j]), (o1[j], a1[j])):
            xs = [cc * v for v in centred(deg(a), q)]
            exact_ties += sum(1 for x in xs if (2 * t * abs(x) + q) % (2 * q) == 0 and x < 0)
            assert np.array_equal(out, circ([round_q(x, q, t) for x in xs], q)), (j, c)
    if any(r == 0 for c in cs for _, r in tie_values(q, t, c)):
        assert exact_ties > 0   # negative exact ties were rounded (the Q - 1 of EV_ROUND)
    want0, want1 = ref_mul(params, a0[0], a1[0], b0[0], b1[0], rlk0, rlk1, w)   # the same by the general oracle
    assert np.array_equal(o0[0], want0) and np.array_equal(o1[0], want1)


@pytest.mark.parametrize("q,t", TIE_PARAMS)
def test_decrypt_and_noise_at_ties(ctx, q, t):
    # row 0: c1 = 0, c0 = x; row 1: c1 random, c0 = x - c1 s; x at and around the ties of round(T x / Q)
    n = 128
    params = (n, q, t, 1)
    rng = np.random.default_rng(q % 99991 + t)
    sk, _, _ = ctx.bfv_fhe_keypair(params, b"\x75" * 32)
    xs = samples([a for a, _ in tie_values(q, t)] + [0, 1, -1, q // 2, q // 2 + 1, q - 1], n, rng, q)
    x = np.array([v % q for v in xs], dtype=object)
    c1 = np.stack([np.zeros(n, dtype=np.uint64), residues(rng, n, q)])
    c0 = np.stack([np.array(x, dtype=np.uint64), np.array((x - c1_times_s(c1[1], sk, q)) % q, dtype=np.uint64)])
    dec = ctx.bfv_decrypt(params, sk, c0, c1)
    want = np.array([decrypt_value(v, q, t) for v in x], dtype=np.uint64)
    assert np.array_equal(dec[0], want) and np.array_equal(dec[1], want)
    noise = ctx.bfv_noise(params, sk, c0, c1)
    assert [int(v) for v in noise] == host_noise(params, sk, c0, c1)
    delta = q // t
    worst = max(min(e, q - e) for e in ((v - delta * centred([int(d)], q)[0]) % q for v, d in zip(x, want)))
    assert int(noise[0]) == int(noise[1]) == worst


# ---- 3. relinearization digits ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [Q63, Q60, Q62])
def test_relin_recomposition_every_width(ctx, q):
    # rlk0_i = 2^(i w) mod Q, rlk1_i = 0: sum_i d_i 2^(i w) = c^2, so out0 = c^0 + c^2 and out1 = c^1 for any inputs.  T = Q - 1
    # makes c^2 = v for 0 <= v < Q/2 and c^2 = Q - 1 for v = -1 when pair 0 is a0 = 0, a1 = 1, b1 = v.
    n = 256
    params = (n, q, q - 1, 19)
    rng = np.random.default_rng(q % 1009)
    for w in range(1, 33):
        l = relin_digits(q, w)
        rlk0 = np.stack([const_poly(n, pow(2, i * w, q), q) for i in range(l)])
        rlk1 = np.zeros((l, n), dtype=np.uint64)
        vs = [0, 1, -1, (1 << w) - 1, 1 << w, (1 << w) + 1, q // 2, -(q // 2), -(1 << w)]
        for k in range(1, l + 1):
            vs += [v for v in ((1 << (k * w)) - 1, 1 << (k * w), ((1 << w) - 1) << ((k - 1) * w)) if v < q // 2]
        b1 = np.stack([circ(samples(vs, n, rng, q), q), residues(rng, n, q)])
        a0 = np.stack([np.zeros(n, dtype=np.uint64), residues(rng, n, q)])
        a1 = np.stack([const_poly(n, 1, q), residues(rng, n, q)])
        b0 = residues(rng, (2, n), q)
        o0, o1 = ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
        for j in range(2):
            c0h, c1h, c2h = ref_tensor(params, a0[j], a1[j], b0[j], b1[j])
            if j == 0:
                assert {0, q - 1, (1 << w) - 1, 1 << w} <= set(c2h), w
            assert np.array_equal(o0[j], circ([x + y for x, y in zip(c0h, c2h)], q)), (w, j)
            assert np.array_equal(o1[j], circ(c1h, q)), (w, j)


@pytest.mark.parametrize("q", [Q63, Q62])
@pytest.mark.parametrize("w", [1, 7, 13, 31])
def test_mul_random_keys_odd_widths(ctx, q, w):
    n = 1024
    params = (n, q, 65537, 19)
    rng = np.random.default_rng(q % 7919 + w)
    l = relin_digits(q, w)
    rlk0, rlk1 = residues(rng, (l, n), q), residues(rng, (l, n), q)
    a0, a1, b0, b1 = (residues(rng, (2, n), q) for _ in range(4))
    o0, o1 = ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    for j in range(2):
        want0, want1 = ref_mul(params, a0[j], a1[j], b0[j], b1[j], rlk0, rlk1, w)
        assert np.array_equal(o0[j], want0) and np.array_equal(o1[j], want1), j


@pytest.mark.parametrize("n,q,t,w", [(64, Q63, 65537, 1), (64, Q62, 1 << 20, 1), (64, Q62, 1 << 20, 31), (1024, Q62, 1 << 20, 16)])
def test_relin_key_restated_at_edges(ctx, n, q, t, w):
    params = (n, q, t, 19)
    sk, _, _ = ctx.bfv_fhe_keypair(params, b"\x76" * 32)
    seed = bytes(range(90, 122))
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed, base_bits=w)
    restate_relin_key(params, sk, seed, w, rlk0, rlk1)


# ---- 4. parameter corners and small rings ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 16, 64, 512])
def test_small_rings_every_call(ctx, n):
    params, w = (n, Q60, 257, 19), 16   # T small enough that products decrypt
    q, t = params[1], params[2]
    rng = np.random.default_rng(n)
    m = random_m(rng, (4, n), q, t)
    sk, pk0, pk1, ct = restate_keypair_and_encryption(ctx, params, bytes([n % 256]) * 32, bytes([n % 256 + 1]) * 32, m)
    c0, c1 = ct["c0"], ct["c1"]
    assert np.array_equal(ctx.bfv_decrypt(params, sk, c0, c1), m)
    for j in range(4):
        assert np.array_equal(ctx.bfv_decrypt(params, sk, c0[j], c1[j])[0], decrypt_formula(params, sk, c0[j], c1[j])), j
    # poly_mul_ternary, both modes
    per = ctx.poly_mul_ternary_negacyclic(c0, ct["u"], q)
    shared = ctx.poly_mul_ternary_negacyclic(pk1, ct["u"], q)
    for j in range(4):
        assert np.array_equal(per[j], negacyclic(c0[j], ct["u"][j], q)) and np.array_equal(shared[j], negacyclic(pk1, ct["u"][j], q)), j
    # add, subtract, sum
    for subtract in (False, True):
        o0, o1 = ctx.bfv_add(params, c0[:2], c1[:2], c0[2:], c1[2:], subtract=subtract)
        sign = -1 if subtract else 1
        assert np.array_equal(obj(o0), (obj(c0[:2]) + sign * obj(c0[2:])) % q) and np.array_equal(obj(o1), (obj(c1[:2]) + sign * obj(c1[2:])) % q)
        assert np.array_equal(ctx.bfv_decrypt(params, sk, o0, o1), as_plain(centred_obj(m[:2], q) + sign * centred_obj(m[2:], q), params))
    s0, s1 = ctx.bfv_sum(params, c0, c1)
    assert np.array_equal(obj(s0), obj(c0).sum(axis=0) % q) and np.array_equal(obj(s1), obj(c1).sum(axis=0) % q)
    assert np.array_equal(ctx.bfv_decrypt(params, sk, s0, s1)[0], as_plain(centred_obj(m, q).sum(axis=0), params))
    # plaintext operations, both modes
    pm = random_m(rng, (4, n), q, t)
    for shared_m in (True, False):
        mm = pm[0] if shared_m else pm
        a0, a1 = ctx.bfv_add_plain(params, c0, c1, mm)
        p0, p1 = ctx.bfv_mul_plain(params, c0, c1, mm)
        assert np.array_equal(a1, c1)
        for j in range(4):
            mj = pm[0] if shared_m else pm[j]
            assert np.array_equal(obj(a0[j]), (obj(c0[j]) + centred_obj(mj, q) * (q // t)) % q), j
            mc = centred(deg(mj), q)
            assert np.array_equal(p0[j], circ(kron_negacyclic([(centred(deg(c0[j]), q), mc)], n), q)), j
            assert np.array_equal(p1[j], circ(kron_negacyclic([(centred(deg(c1[j]), q), mc)], n), q)), j
            assert np.array_equal(ctx.bfv_decrypt(params, sk, a0[j], a1[j])[0], as_plain(centred_obj(m[j], q) + centred_obj(mj, q), params)), j
            assert np.array_equal(ctx.bfv_decrypt(params, sk, p0[j], p1[j])[0], plain_product(m[j], mj, params)), j
    # the relinearization key and products
    seed = b"\x77" * 32
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed, base_bits=w)
    restate_relin_key(params, sk, seed, w, rlk0, rlk1)
    o0, o1 = ctx.bfv_mul(params, c0[:2], c1[:2], c0[2:], c1[2:], rlk0, rlk1, base_bits=w)
    for j in range(2):
        want0, want1 = ref_mul(params, c0[j], c1[j], c0[2 + j], c1[2 + j], rlk0, rlk1, w)
        assert np.array_equal(o0[j], want0) and np.array_equal(o1[j], want1), j
        assert np.array_equal(ctx.bfv_decrypt(params, sk, o0[j], o1[j])[0], plain_product(m[j], m[2 + j], params)), j
    for x0, x1 in ((c0, c1), (o0, o1), (s0[None], s1[None])):
        assert [int(v) for v in ctx.bfv_noise(params, sk, x0, x1)] == host_noise(params, sk, x0, x1)


@pytest.mark.parametrize("params", [(8, 3, 2, 1), (16, Q62, 1 << 20, 19)])
def test_tiny_parameters(ctx, params):
    # at Q = 3 decryption is not expected to be right: the samples and the defining formulas are checked instead
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(q % 1000)
    m = random_m(rng, (3, n), q, t)
    sk, pk0, pk1, ct = restate_keypair_and_encryption(ctx, params, b"\x78" * 32, b"\x79" * 32, m, first=5)
    c0, c1 = ct["c0"], ct["c1"]
    dec = ctx.bfv_decrypt(params, sk, c0, c1)
    for j in range(3):
        assert np.array_equal(dec[j], decrypt_formula(params, sk, c0[j], c1[j])), j
    if q > 3:
        assert np.array_equal(dec, m)
    assert [int(v) for v in ctx.bfv_noise(params, sk, c0, c1)] == host_noise(params, sk, c0, c1)
    for w in (1, 2, 32):
        seed = bytes([w]) * 32
        rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed, base_bits=w)
        restate_relin_key(params, sk, seed, w, rlk0, rlk1)
        a0, a1, b0, b1 = (residues(rng, (2, n), q) for _ in range(4))
        o0, o1 = ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
        for j in range(2):
            want0, want1 = ref_mul(params, a0[j], a1[j], b0[j], b1[j], rlk0, rlk1, w)
            assert np.array_equal(o0[j], want0) and np.array_equal(o1[j], want1), (w, j)
        assert [int(v) for v in ctx.bfv_noise(params, sk, o0, o1)] == host_noise(params, sk, o0, o1)
    a0, a1 = ctx.bfv_add_plain(params, c0, c1, m)
    p0, p1 = ctx.bfv_mul_plain(params, c0, c1, m[0])
    for j in range(3):
        assert np.array_equal(obj(a0[j]), (obj(c0[j]) + centred_obj(m[j], q) * (q // t)) % q), j
        mc = centred(deg(m[0]), q)
        assert np.array_equal(p0[j], circ(kron_negacyclic([(centred(deg(c0[j]), q), mc)], n), q)), j
        assert np.array_equal(p1[j], circ(kron_negacyclic([(centred(deg(c1[j]), q), mc)], n), q)), j
    s0, s1 = ctx.bfv_sum(params, c0, c1)
    assert np.array_equal(obj(s0), obj(c0).sum(axis=0) % q) and np.array_equal(obj(s1), obj(c1).sum(axis=0) % q)


@pytest.mark.parametrize("t", [2, Q60 // 2 - 1])
def test_small_and_half_q_plaintext_modulus(ctx, t):
    # T = 2 decrypts products correctly; T = floor(Q/2) - 1 (even, delta = 2) is checked against the formulas
    n, w = 1024, 32
    params = (n, Q60, t, 19)
    q = params[1]
    assert t % 2 == 0
    rng = np.random.default_rng(t % 1000)
    m = random_m(rng, (4, n), q, t)
    sk, pk0, pk1, ct = restate_keypair_and_encryption(ctx, params, b"\x7a" * 32, b"\x7b" * 32, m)
    c0, c1 = ct["c0"], ct["c1"]
    dec = ctx.bfv_decrypt(params, sk, c0, c1)
    for j in range(4):
        assert np.array_equal(dec[j], decrypt_formula(params, sk, c0[j], c1[j])), j
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, b"\x7c" * 32, base_bits=w)
    o0, o1 = ctx.bfv_mul(params, c0[:2], c1[:2], c0[2:], c1[2:], rlk0, rlk1, base_bits=w)
    for j in range(2):
        want0, want1 = ref_mul(params, c0[j], c1[j], c0[2 + j], c1[2 + j], rlk0, rlk1, w)
        assert np.array_equal(o0[j], want0) and np.array_equal(o1[j], want1), j
    pm = random_m(rng, (4, n), q, t)
    a0, a1 = ctx.bfv_add_plain(params, c0, c1, pm)
    p0, p1 = ctx.bfv_mul_plain(params, c0, c1, pm)
    for j in range(4):
        assert np.array_equal(obj(a0[j]), (obj(c0[j]) + centred_obj(pm[j], q) * (q // t)) % q), j
        mc = centred(deg(pm[j]), q)
        assert np.array_equal(p0[j], circ(kron_negacyclic([(centred(deg(c0[j]), q), mc)], n), q)), j
        assert np.array_equal(p1[j], circ(kron_negacyclic([(centred(deg(c1[j]), q), mc)], n), q)), j
    for x0, x1 in ((c0, c1), (o0, o1), (a0, a1)):
        assert [int(v) for v in ctx.bfv_noise(params, sk, x0, x1)] == host_noise(params, sk, x0, x1)
    if t == 2:
        assert np.array_equal(dec, m)
        for j in range(2):
            assert np.array_equal(ctx.bfv_decrypt(params, sk, o0[j], o1[j])[0], plain_product(m[j], m[2 + j], params)), j
            assert np.array_equal(ctx.bfv_decrypt(params, sk, p0[j], p1[j])[0], plain_product(m[j], pm[j], params)), j
            assert np.array_equal(ctx.bfv_decrypt(params, sk, a0[j], a1[j])[0], as_plain(centred_obj(m[j], q) + centred_obj(pm[j], q), params)), j


def test_error_bound_1023(ctx):
    # B = 1023: the sampler's full 2046-threshold table (16 KiB of LDS) in key generation, encryption and the relinearization key
    n, w = 1024, 32
    params = (n, Q60, 65537, 1023)
    q, t = params[1], params[2]
    m = random_m(np.random.default_rng(1023), (3, n), q, t)
    sk, pk0, pk1, ct = restate_keypair_and_encryption(ctx, params, b"\x7d" * 32, b"\x7e" * 32, m, first=1 << 40)
    assert np.array_equal(ctx.bfv_decrypt(params, sk, ct["c0"], ct["c1"]), m)
    seed = b"\x7f" * 32
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed, base_bits=w)
    restate_relin_key(params, sk, seed, w, rlk0, rlk1)


def test_mul_plain_crt_bound_at_the_edge(ctx):
    # |c| = floor(Q/2), |m| = floor(T/2) with T = Q - 2 at N = 32768: |c m| sums to N floor(Q/2) floor(T/2) ~ 2^139
    n, q = 32768, Q63
    t = q - 2
    params = (n, q, t, 1)
    h, k = q // 2, t // 2
    assert (n * h * k).bit_length() == 139
    plus = lambda v, s: np.full(n, v if s > 0 else q - v, dtype=np.uint64)  # noqa: E731
    rng = np.random.default_rng(32768)
    rand_c = np.where(rng.integers(0, 2, n) == 1, np.uint64(h), np.uint64(q - h)).astype(np.uint64)
    rand_m = np.where(rng.integers(0, 2, n) == 1, np.uint64(k), np.uint64(q - k)).astype(np.uint64)
    c0 = np.stack([plus(h, 1), rand_c])
    c1 = np.stack([plus(h, -1), plus(h, -1)])

    def coeff(a, b, d):   # degree d of the negacyclic product, schoolbook on Python integers
        return np.dot(a[:d + 1], b[d::-1]) - (np.dot(a[d + 1:], b[n - 1:d:-1]) if d < n - 1 else 0)

    for shared in (True, False):
        mm = plus(k, 1) if shared else np.stack([plus(k, -1), rand_m])
        o0, o1 = ctx.bfv_mul_plain(params, c0, c1, mm)
        s_m = 1 if shared else -1
        # constant polynomials: degree d of (s_a h)(s_b k) (sum over x^i x^j) = s_a s_b h k (2d + 2 - N)
        assert np.array_equal(o0[0], circ([s_m * h * k * (2 * d + 2 - n) for d in range(n)], q))
        assert np.array_equal(o1[0], circ([-s_m * h * k * (2 * d + 2 - n) for d in range(n)], q))
        M = np.array(centred(deg(mm if shared else mm[1]), q), dtype=object)
        for out, c in ((o0[1], c0[1]), (o1[1], c1[1])):
            C = np.array(centred(deg(c), q), dtype=object)
            for d in sorted(set(rng.integers(0, n, 16).tolist()) | {0, n - 1}):
                assert int(out[n - 1 - d]) == coeff(C, M, d) % q, (shared, d)


@pytest.mark.parametrize("q,t", [(Q63, Q63 - 2), (Q62, Q62 - 1)])
def test_noise_and_decrypt_with_t_near_q(ctx, q, t):
    n = 1024
    params = (n, q, t, 19)
    rng = np.random.default_rng(t % 1000)
    sk, _, _ = ctx.bfv_fhe_keypair(params, b"\x80" * 32)
    c0, c1 = residues(rng, (3, n), q), residues(rng, (3, n), q)
    c0[2] = circ(samples([a for a, _ in tie_values(q, t)] + [0, q // 2, q // 2 + 1, q - 1], n, rng, q), q)
    c1[2] = 0
    assert [int(v) for v in ctx.bfv_noise(params, sk, c0, c1)] == host_noise(params, sk, c0, c1)
    dec = ctx.bfv_decrypt(params, sk, c0, c1)
    for j in range(3):
        assert np.array_equal(dec[j], decrypt_formula(params, sk, c0[j], c1[j])), j
