"""BFV slots and rotations on the GPU (bfv_galois.hip): encode / decode, Galois keys, key switches and slot_sum bit for bit against
the restatements of tests/test_bfv_galois_host.py, decryption of rotated and row-swapped slots, slot-wise products through the
existing mul_plain and mul, collective Galois keys opening a slot-summed tally by threshold decryption, and every refusal.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60, relin_digits
from tests.test_bfv_galois_host import (encode, eval_slots, galois_element, plain_slot_sum, ref_apply_galois, ref_galois_key, rotate,
                                        sigma, slot_sum_elements)

pytestmark = pytest.mark.gpu
K13 = (1024, Q29, 7, 19)             # the k = 13 parameters: no batching (T = 7)
B1024 = (1024, Q60, 12289, 19)       # batching at N = 1024
B4096 = (4096, Q60, 65537, 19)
CRS = b"\xc5" * 32
PARTIES = [bytes([0x40 + i]) * 32 for i in range(3)]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def slot_values(rng, params, count=1):
    return rng.integers(0, params[2], size=(count, params[0]), dtype=np.uint64)


def residues(rng, params, count):
    return rng.integers(0, params[1], size=(count, params[0]), dtype=np.uint64)


def keys_for(ctx, params, sk, elements, w, seed=b"\x51" * 32):
    ks = [ctx.bfv_galois_keygen(params, sk, g, seed=seed, base_bits=w) for g in elements]
    return np.array([k[0] for k in ks]), np.array([k[1] for k in ks])


# ---- 1. encode / decode ----------------------------------------------------------------------------------------------------

def test_encode_decode_restated_1024(ctx):
    rng = np.random.default_rng(1)
    v = slot_values(rng, B1024, 3)
    m = ctx.bfv_encode_slots(B1024, v)
    for j in range(3):
        assert np.array_equal(m[j], encode(B1024, v[j])), j
    assert np.array_equal(ctx.bfv_decode_slots(B1024, m), v)
    # decode of an arbitrary plaintext in range, against the evaluation restated
    t, q = B1024[2], B1024[1]
    x = rng.integers(-(t // 2), t // 2 + 1, size=B1024[0])
    p = np.array([int(a) % q for a in x], dtype=np.uint64)
    assert np.array_equal(ctx.bfv_decode_slots(B1024, p)[0], eval_slots(B1024, p))
    ends = np.array([[0] * 512 + [t - 1] * 512], dtype=np.uint64)
    assert np.array_equal(ctx.bfv_decode_slots(B1024, ctx.bfv_encode_slots(B1024, ends)), ends)


@pytest.mark.parametrize("n", [4096, 32768])
def test_encode_decode_round_trip_and_spot_values(ctx, n):
    params = (n, Q60, 65537, 19)
    rng = np.random.default_rng(n)
    v = slot_values(rng, params, 2)
    m = ctx.bfv_encode_slots(params, v)
    assert np.array_equal(ctx.bfv_decode_slots(params, m), v)
    q, t = params[1], params[2]
    assert all(int(x) <= t // 2 or int(x) >= q - t // 2 for x in m[1])
    spots = [0, 1, n // 2 - 1, n // 2, n - 1, 12345 % n]
    assert np.array_equal(eval_slots(params, m[1], spots), v[1][spots])


# ---- 2. keys -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", [(K13, 4), (B4096, 16)])
def test_galois_keygen_restated(ctx, params, w):
    sk = ctx.bfv_fhe_keypair(params, b"\x50" * 32)[0]
    n = params[0]
    for g in (1, galois_element(n, 3), 2 * n - 1):
        gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=b"\x51" * 32, base_bits=w)
        r, a = ref_galois_key(params, sk, b"\x51" * 32, b"\x51" * 32, g, w)
        assert gk0.shape == (relin_digits(params[1], w), n)
        assert np.array_equal(gk0, r) and np.array_equal(gk1, a), g


def test_one_party_galois_share_is_galois_keygen(ctx):
    params = B1024
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    g = galois_element(params[0], 5)
    seed = bytes(range(32))
    r, a = ctx.bfv_galois_share(params, sk, seed, seed, g, base_bits=12)
    gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=seed, base_bits=12)
    assert np.array_equal(r, gk0) and np.array_equal(a, gk1)
    r, a = ctx.bfv_galois_share(params, sk, CRS, PARTIES[1], g, base_bits=12)
    rr, ra = ref_galois_key(params, sk, CRS, PARTIES[1], g, 12)
    assert np.array_equal(r, rr) and np.array_equal(a, ra)


# ---- 3. key switch -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", [(K13, 4), (B4096, 16)])
def test_apply_galois_restated(ctx, params, w):
    n = params[0]
    rng = np.random.default_rng(7)
    sk = ctx.bfv_fhe_keypair(params, b"\x52" * 32)[0]
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    for g in (1, 5, galois_element(n, -7), 2 * n - 1):
        gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=b"\x53" * 32, base_bits=w)
        o0, o1 = ctx.bfv_apply_galois(params, c0, c1, g, gk0, gk1, base_bits=w)
        for j in range(2):
            r0, r1 = ref_apply_galois(params, c0[j], c1[j], g, gk0, gk1, w)
            assert np.array_equal(o0[j], r0) and np.array_equal(o1[j], r1), (g, j)


def test_apply_galois_across_a_chunk(ctx):
    """2049 ciphertexts at N = 1024: one more than chunk_polys(N)"""
    params = K13
    rng = np.random.default_rng(8)
    count = 2049
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    sk = ctx.bfv_fhe_keypair(params, b"\x54" * 32)[0]
    g = 2 * params[0] - 3
    gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=b"\x55" * 32, base_bits=8)
    o0, o1 = ctx.bfv_apply_galois(params, c0, c1, g, gk0, gk1, base_bits=8)
    for j in (0, 2047, 2048):
        r0, r1 = ref_apply_galois(params, c0[j], c1[j], g, gk0, gk1, 8)
        assert np.array_equal(o0[j], r0) and np.array_equal(o1[j], r1), j


def test_rotations_decrypt(ctx):
    params = B4096
    n, q, t = params[0], params[1], params[2]
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x56" * 32)
    rng = np.random.default_rng(9)
    v = slot_values(rng, params, 1)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\x57" * 32)
    for steps, swap in ((1, False), (-3, False), (0, True), (100, True)):
        g = galois_element(n, steps, swap)
        gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=b"\x58" * 32, base_bits=16)
        o0, o1 = ctx.bfv_apply_galois(params, ct["c0"], ct["c1"], g, gk0, gk1, base_bits=16)
        got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, o0, o1))
        assert np.array_equal(got[0], rotate(v[0], steps % (n // 2), swap)), (steps, swap)
        assert int(ctx.bfv_noise(params, sk, o0, o1)[0]) < (q // t) // 2


def test_sigma_on_coefficients_decrypts(ctx):
    params = K13
    n, q, t = params[0], params[1], params[2]
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x59" * 32)
    rng = np.random.default_rng(10)
    m = np.array([int(x) % q for x in rng.integers(-3, 4, size=n)], dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x5a" * 32)
    for g in (1, 3, 5, 2 * n - 1):
        gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=b"\x5b" * 32, base_bits=4)
        o0, o1 = ctx.bfv_apply_galois(params, ct["c0"], ct["c1"], g, gk0, gk1, base_bits=4)
        assert np.array_equal(ctx.bfv_decrypt(params, sk, o0, o1)[0], sigma(m, g, q)), g
        assert int(ctx.bfv_noise(params, sk, o0, o1)[0]) < (q // t) // 2


# ---- 4. slot-wise products ---------------------------------------------------------------------------------------------------

def test_slot_wise_products(ctx):
    params = B1024
    q, t = params[1], params[2]
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x5c" * 32)
    rng = np.random.default_rng(11)
    a, b = slot_values(rng, params, 1), slot_values(rng, params, 1)
    want = (a.astype(object) * b.astype(object) % t).astype(np.uint64)
    ma, mb = ctx.bfv_encode_slots(params, a), ctx.bfv_encode_slots(params, b)
    ca = ctx.bfv_encrypt(params, pk0, pk1, ma, b"\x5d" * 32)
    cb = ctx.bfv_encrypt(params, pk0, pk1, mb, b"\x5e" * 32)
    p0, p1 = ctx.bfv_mul_plain(params, ca["c0"], ca["c1"], mb)
    assert np.array_equal(ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, p0, p1)), want)
    noise_plain = int(ctx.bfv_noise(params, sk, p0, p1)[0])
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed=b"\x5f" * 32, base_bits=16)
    x0, x1 = ctx.bfv_mul(params, ca["c0"], ca["c1"], cb["c0"], cb["c1"], rlk0, rlk1, base_bits=16)
    assert np.array_equal(ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, x0, x1)), want)
    noise_mul = int(ctx.bfv_noise(params, sk, x0, x1)[0])
    limit = (q // t) // 2
    print("slot-wise product noise: mul_plain 2^%.1f, mul 2^%.1f, limit 2^%.1f"
          % (np.log2(max(noise_plain, 1)), np.log2(max(noise_mul, 1)), np.log2(limit)))
    assert noise_plain < limit and noise_mul < limit


# ---- 5. slot_sum -----------------------------------------------------------------------------------------------------------

def test_slot_sum_is_the_composition_and_totals(ctx):
    params = B1024
    n, q, t = params[0], params[1], params[2]
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x60" * 32)
    rng = np.random.default_rng(12)
    v = slot_values(rng, params, 2)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\x61" * 32)
    import zk_fhe_amd as zk
    elements = zk.bfv_slot_sum_elements(params)
    assert elements == slot_sum_elements(n)
    gk0, gk1 = keys_for(ctx, params, sk, elements, 16)
    s0, s1 = ctx.bfv_slot_sum(params, ct["c0"], ct["c1"], gk0, gk1, base_bits=16)
    x0, x1 = ct["c0"], ct["c1"]
    for k, g in enumerate(elements):
        r0, r1 = ctx.bfv_apply_galois(params, x0, x1, g, gk0[k], gk1[k], base_bits=16)
        x0, x1 = ctx.bfv_add(params, x0, x1, r0, r1)
    assert np.array_equal(s0, x0) and np.array_equal(s1, x1)
    m = ctx.bfv_decrypt(params, sk, s0, s1)
    totals = v.astype(object).sum(axis=1) % t
    for j in range(2):
        assert np.array_equal(ctx.bfv_decode_slots(params, m[j])[0], np.full(n, totals[j], dtype=np.uint64))
    assert np.array_equal(m[0], plain_slot_sum(params, ctx.bfv_encode_slots(params, v[0])[0]))
    assert int(ctx.bfv_noise(params, sk, s0, s1).max()) < (q // t) // 2
    # defined for any T: the composition at the k = 13 parameters, one ciphertext
    sk7 = ctx.bfv_fhe_keypair(K13, b"\x62" * 32)[0]
    e7 = zk.bfv_slot_sum_elements(K13)
    g0, g1 = keys_for(ctx, K13, sk7, e7, 8)
    c0, c1 = residues(rng, K13, 1), residues(rng, K13, 1)
    s0, s1 = ctx.bfv_slot_sum(K13, c0, c1, g0, g1, base_bits=8)
    for k, g in enumerate(e7):
        r0, r1 = ctx.bfv_apply_galois(K13, c0, c1, g, g0[k], g1[k], base_bits=8)
        c0, c1 = ctx.bfv_add(K13, c0, c1, r0, r1)
    assert np.array_equal(s0, c0) and np.array_equal(s1, c1)


# ---- 6. threshold --------------------------------------------------------------------------------------------------------------

def test_threshold_slot_sum_tally(ctx):
    import zk_fhe_amd as zk
    params = B1024
    n, q, t = params[0], params[1], params[2]
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES]
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]
    w = 8
    elements = zk.bfv_slot_sum_elements(params)
    gk0, gk1 = [], []
    for g in elements:
        shares = [ctx.bfv_galois_share(params, sk, CRS, ps, g, base_bits=w) for sk, ps in zip(sks, PARTIES)]
        assert all(np.array_equal(s[1], shares[0][1]) for s in shares)   # one CRS a_j
        gk0.append(ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])))
        gk1.append(shares[0][1])
    gk0, gk1 = np.array(gk0), np.array(gk1)
    rng = np.random.default_rng(13)
    ballots = rng.integers(0, 2, size=(5, n), dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, ballots), b"\x63" * 32)
    c0, c1 = ctx.bfv_sum(params, ct["c0"], ct["c1"])
    s0, s1 = ctx.bfv_slot_sum(params, c0, c1, gk0, gk1, base_bits=w)
    shares = [ctx.bfv_decrypt_share(params, sk, s1, seed=bytes([0x70, i]) * 16, smudge_bound=1 << 20) for i, sk in enumerate(sks)]
    m = ctx.bfv_decrypt_combine(params, s0, np.array(shares))
    total = int(ballots.sum()) % t
    assert np.array_equal(ctx.bfv_decode_slots(params, m)[0], np.full(n, total, dtype=np.uint64))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import zk_fhe_amd as zk
    params = B1024
    n, q, t = params[0], params[1], params[2]
    sk = ctx.bfv_fhe_keypair(params, b"\x64" * 32)[0]
    z = np.zeros((1, n), dtype=np.uint64)
    gk0, gk1 = ctx.bfv_galois_keygen(params, sk, 5, seed=b"\x65" * 32, base_bits=16)
    with pytest.raises(zk.ZkfheError, match="batching"):
        ctx.bfv_encode_slots(K13, z)
    with pytest.raises(zk.ZkfheError, match="batching"):
        ctx.bfv_decode_slots((1024, Q60, 13313, 19), z)
    bad = z.copy()
    bad[0, 9] = t
    with pytest.raises(zk.ZkfheError, match="not below T"):
        ctx.bfv_encode_slots(params, bad)
    bad[0, 9] = t // 2 + 1
    with pytest.raises(zk.ZkfheError, match="outside"):
        ctx.bfv_decode_slots(params, bad)
    for g in (0, 4, 2 * n, 2 * n + 1):
        with pytest.raises(zk.ZkfheError, match="odd and below 2N"):
            ctx.bfv_apply_galois(params, z, z, g, gk0, gk1)
        with pytest.raises(zk.ZkfheError, match="odd and below 2N"):
            ctx.bfv_galois_keygen(params, sk, g, seed=b"\x65" * 32)
        with pytest.raises(zk.ZkfheError, match="odd and below 2N"):
            ctx.bfv_galois_share(params, sk, CRS, PARTIES[0], g)
    big = z.copy()
    big[0, 3] = q
    with pytest.raises(zk.ZkfheError, match="ciphertext"):
        ctx.bfv_apply_galois(params, big, z, 5, gk0, gk1)
    with pytest.raises(zk.ZkfheError, match="ciphertext"):
        ctx.bfv_slot_sum(params, z, big, np.zeros((10,) + gk0.shape, np.uint64), np.zeros((10,) + gk0.shape, np.uint64))
    bk = gk1.copy()
    bk[1, 2] = q
    with pytest.raises(zk.ZkfheError, match="Galois-key"):
        ctx.bfv_apply_galois(params, z, z, 5, gk0, bk)
    with pytest.raises(zk.ZkfheError, match="Galois-key"):
        ctx.bfv_slot_sum(params, z, z, np.zeros((10,) + gk0.shape, np.uint64), np.broadcast_to(bk, (10,) + bk.shape))
    bsk = sk.copy()
    bsk[4] = 2
    with pytest.raises(zk.ZkfheError, match="secret-key"):
        ctx.bfv_galois_keygen(params, bsk, 5, seed=b"\x65" * 32)
    with pytest.raises(zk.ZkfheError, match="secret-key"):
        ctx.bfv_galois_share(params, bsk, CRS, PARTIES[0], 5)
    for w in (0, 33):
        with pytest.raises(zk.ZkfheError, match="base_bits"):
            ctx.bfv_galois_keygen(params, sk, 5, seed=b"\x65" * 32, base_bits=w)
        with pytest.raises(zk.ZkfheError, match="base_bits"):
            ctx.bfv_galois_share(params, sk, CRS, PARTIES[0], 5, base_bits=w)
        with pytest.raises(zk.ZkfheError, match="base_bits"):
            ctx.bfv_apply_galois(params, z, z, 5, gk0, gk1, base_bits=w)
        with pytest.raises(zk.ZkfheError, match="base_bits"):
            ctx.bfv_slot_sum(params, z, z, np.zeros((10,) + gk0.shape, np.uint64), np.zeros((10,) + gk0.shape, np.uint64), base_bits=w)
    # n = 0 and NULL pointers, at the C boundary
    import ctypes
    u64p = ctypes.POINTER(ctypes.c_uint64)
    prm = zk.BfvParamsC(*params)
    lib = ctx.lib
    buf = np.zeros(n, dtype=np.uint64)
    p = buf.ctypes.data_as(u64p)
    for fn in (lib.zkfhe_bfv_encode_slots, lib.zkfhe_bfv_decode_slots):
        assert fn(ctx.h, ctypes.byref(prm), 0, p, p) != 0
        assert fn(ctx.h, ctypes.byref(prm), 1, None, p) != 0
        assert fn(ctx.h, ctypes.byref(prm), 1, p, None) != 0
    gp = gk0.ctypes.data_as(u64p)
    assert lib.zkfhe_bfv_apply_galois(ctx.h, ctypes.byref(prm), 0, p, p, 5, gp, gp, 16, p, p) != 0
    assert lib.zkfhe_bfv_apply_galois(ctx.h, ctypes.byref(prm), 1, p, p, 5, None, gp, 16, p, p) != 0
    assert lib.zkfhe_bfv_slot_count(ctypes.byref(prm), None) != 0
    assert lib.zkfhe_bfv_galois_element(ctypes.byref(prm), 1, 0, None) != 0
