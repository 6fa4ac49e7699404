"""Hoisted BFV rotations and slot-wise linear transforms on the GPU (bfv_linear.hip): both calls bit for bit against the restatements
of tests/test_bfv_linear_host.py, across a chunk, linear_transform against the composition through the existing GPU calls,
decrypted matrix-vector products of banded matrices under a single key and under a three-party collective key, and every refusal.
Run on the MI355X box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60, Q63, relin_digits
from tests.test_bfv_galois_host import galois_element
from tests.test_bfv_linear_host import ref_hoisted_rotation, ref_linear_transform

pytestmark = pytest.mark.gpu
A1024 = (1024, Q29, 12289, 19)
B1024 = (1024, Q60, 12289, 19)
B4096 = (4096, Q60, 65537, 19)
CRS = b"\xc6" * 32
PARTIES = [bytes([0x48 + i]) * 32 for i in range(3)]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def residues(rng, params, count):
    return rng.integers(0, params[1], size=(count, params[0]), dtype=np.uint64)


def plaintexts(rng, params, count):
    """random plaintexts over the whole range [0, T/2] and [Q - T/2, Q - 1]"""
    q, t = params[1], params[2]
    x = rng.integers(-(t // 2), t // 2 + 1, size=(count, params[0]))
    return np.array([[int(a) % q for a in row] for row in x], dtype=np.uint64)


def keys_for(ctx, params, sk, elements, w, seed=b"\x81" * 32):
    ks = [ctx.bfv_galois_keygen(params, sk, g, seed=seed, base_bits=w) for g in elements]
    return np.array([k[0] for k in ks]), np.array([k[1] for k in ks])


def six_elements(n):
    """g = 1, two rotations (one of them twice), the row swap and a swapped rotation"""
    return [galois_element(n, 1), 1, 2 * n - 1, galois_element(n, -7), galois_element(n, 1), galois_element(n, 40, True)]


# ---- 1. both calls, restated ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", [(A1024, 4), (B4096, 16)])
def test_both_calls_restated(ctx, params, w):
    n = params[0]
    rng = np.random.default_rng(21)
    sk = ctx.bfv_fhe_keypair(params, b"\x80" * 32)[0]
    elements = six_elements(n)
    gk0, gk1 = keys_for(ctx, params, sk, elements, w)
    c0, c1 = residues(rng, params, 3), residues(rng, params, 3)
    o0, o1 = ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w)
    assert o0.shape == o1.shape == (6, 3, n)
    for k, g in enumerate(elements):
        for j in range(3):
            r0, r1 = ref_hoisted_rotation(params, c0[j], c1[j], g, gk0[k], gk1[k], w)
            assert np.array_equal(o0[k, j], r0) and np.array_equal(o1[k, j], r1), (g, j)
    assert np.array_equal(o0[0], o0[4]) and np.array_equal(o1[0], o1[4])   # the repeated element
    diag = plaintexts(rng, params, 6)
    t0, t1 = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    assert t0.shape == t1.shape == (3, n)
    for j in (0, 2):
        r0, r1 = ref_linear_transform(params, c0[j], c1[j], elements, gk0, gk1, w, diag)
        assert np.array_equal(t0[j], r0) and np.array_equal(t1[j], r1), j


# ---- 2. across a chunk ---------------------------------------------------------------------------------------------------------

def test_both_calls_across_a_chunk(ctx):
    """230 ciphertexts at N = 1024, w = 4: l + 1 = 9 hoisted rows per ciphertext, so a chunk holds chunk_polys(N) / 9 = 227"""
    params, w, count = A1024, 4, 230
    n = params[0]
    rng = np.random.default_rng(22)
    sk = ctx.bfv_fhe_keypair(params, b"\x82" * 32)[0]
    elements = [galois_element(n, 3), 1, 2 * n - 3]
    gk0, gk1 = keys_for(ctx, params, sk, elements, w)
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    diag = plaintexts(rng, params, 3)
    o0, o1 = ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w)
    t0, t1 = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    for j in (0, 225, 226, 227, 229):
        for k, g in enumerate(elements):
            r0, r1 = ref_hoisted_rotation(params, c0[j], c1[j], g, gk0[k], gk1[k], w)
            assert np.array_equal(o0[k, j], r0) and np.array_equal(o1[k, j], r1), (g, j)
        r0, r1 = ref_linear_transform(params, c0[j], c1[j], elements, gk0, gk1, w, diag)
        assert np.array_equal(t0[j], r0) and np.array_equal(t1[j], r1), j


# ---- 3. the composition through the existing calls ----------------------------------------------------------------------------

@pytest.mark.parametrize("params,w,count", [(B1024, 8, 5), (B4096, 16, 2), ((32768, Q60, 65537, 19), 16, 1)])
def test_linear_transform_is_the_composition(ctx, params, w, count):
    n = params[0]
    rng = np.random.default_rng(23)
    sk = ctx.bfv_fhe_keypair(params, b"\x83" * 32)[0]
    elements = six_elements(n)
    gk0, gk1 = keys_for(ctx, params, sk, elements, w)
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    diag = plaintexts(rng, params, 6)
    r0, r1 = ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w)
    acc = None
    for k in range(6):
        p0, p1 = ctx.bfv_mul_plain(params, r0[k], r1[k], diag[k])
        acc = (p0, p1) if acc is None else ctx.bfv_add(params, acc[0], acc[1], p0, p1)
    t0, t1 = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    assert np.array_equal(t0, acc[0]) and np.array_equal(t1, acc[1])


# ---- 4. matrix-vector products -------------------------------------------------------------------------------------------------

def banded(rng, params, offsets, swapped):
    """a random matrix over Z_T in slot order with the diagonals `offsets` inside each row block and `swapped` across the blocks"""
    n, t = params[0], params[2]
    half, p = n // 2, np.arange(n)
    m = np.zeros((n, n), dtype=np.int64)
    for swap, offs in ((0, offsets), (1, swapped)):
        for k in offs:
            m[p, ((p // half) ^ swap) * half + (p % half + k) % half] = rng.integers(1, t, size=n)
    return m


def matvec(params, m, v):
    return (m @ v.astype(np.int64) % params[2]).astype(np.uint64)   # entries below 2^17, N <= 2^12: below 2^46


MATVEC = [(B1024, 8, (0, 1, 2, 5), (0, 3)), (B4096, 4, (0, 1, 2, 3, 100), (0, 1, 7))]   # K = 6 and K = 8 diagonals


@pytest.mark.parametrize("params,w,offsets,swapped", MATVEC)
def test_matrix_vector_product_decrypts(ctx, params, w, offsets, swapped):
    import zk_fhe_amd as zk
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(24)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x84" * 32)
    m = banded(rng, params, offsets, swapped)
    elements, d = zk.bfv_matrix_diagonals(params, m)
    assert len(elements) == len(offsets) + len(swapped) and elements[0] == 1
    gk0, gk1 = keys_for(ctx, params, sk, elements, w)
    v = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\x85" * 32)
    o0, o1 = ctx.bfv_linear_transform(params, ct["c0"], ct["c1"], elements, gk0, gk1, ctx.bfv_encode_slots(params, d), base_bits=w)
    noise, limit = int(ctx.bfv_noise(params, sk, o0, o1).max()), (q // t) // 2
    print("matrix-vector product at N = %d, w = %d, K = %d: noise 2^%.1f, limit 2^%.1f" % (n, w, len(elements), np.log2(max(noise, 1)), np.log2(limit)))
    got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, o0, o1))
    for j in range(2):
        assert np.array_equal(got[j], matvec(params, m, v[j])), j
    assert noise < limit


# ---- 5. under a collective key -------------------------------------------------------------------------------------------------

def test_matrix_vector_product_under_a_collective_key(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 8
    n, t = params[0], params[2]
    rng = np.random.default_rng(25)
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES]
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]
    m = banded(rng, params, (0, 1, 2, 5), (0, 3))
    elements, d = zk.bfv_matrix_diagonals(params, m)
    gk0, gk1 = [], []
    for g in elements:
        shares = [ctx.bfv_galois_share(params, sk, CRS, ps, g, base_bits=w) for sk, ps in zip(sks, PARTIES)]
        gk0.append(ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])))
        gk1.append(shares[0][1])
    gk0, gk1 = np.array(gk0), np.array(gk1)
    v = rng.integers(0, t, size=(1, n), dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\x86" * 32)
    o0, o1 = ctx.bfv_linear_transform(params, ct["c0"], ct["c1"], elements, gk0, gk1, ctx.bfv_encode_slots(params, d), base_bits=w)
    shares = [ctx.bfv_decrypt_share(params, sk, o1, seed=bytes([0x78, i]) * 16, smudge_bound=1 << 20) for i, sk in enumerate(sks)]
    got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt_combine(params, o0, np.array(shares)))
    assert np.array_equal(got[0], matvec(params, m, v[0]))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def both(ctx, params, c0, c1, elements, gk0, gk1, diag, w=16):
    """the two calls on the same arguments, as thunks"""
    return (lambda: ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w),
            lambda: ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w))


def test_refusals(ctx):
    import zk_fhe_amd as zk
    params = B1024
    n, q, t = params[0], params[1], params[2]
    l = relin_digits(q, 16)
    z = np.zeros((1, n), dtype=np.uint64)
    keys = np.zeros((2, l, n), dtype=np.uint64)
    diag = np.zeros((2, n), dtype=np.uint64)
    for g in (0, 4, 2 * n, 2 * n + 1):
        for call in both(ctx, params, z, z, [5, g], keys, keys, diag):
            with pytest.raises(zk.ZkfheError, match="odd and below 2N"):
                call()
    big = z.copy()
    big[0, 3] = q
    for a, b in ((big, z), (z, big)):
        for call in both(ctx, params, a, b, [5, 3], keys, keys, diag):
            with pytest.raises(zk.ZkfheError, match="ciphertext coefficient is not below Q"):
                call()
    bk = keys.copy()
    bk[1, 1, 2] = q
    for a, b in ((bk, keys), (keys, bk)):
        for call in both(ctx, params, z, z, [5, 3], a, b, diag):
            with pytest.raises(zk.ZkfheError, match="Galois-key coefficient is not below Q"):
                call()
    for bad in (t // 2 + 1, q - t // 2 - 1, q):
        bd = diag.copy()
        bd[1, 7] = bad
        with pytest.raises(zk.ZkfheError, match="a diagonal coefficient is outside"):
            ctx.bfv_linear_transform(params, z, z, [5, 3], keys, keys, bd)
    for w in (0, 33):
        for call in both(ctx, params, z, z, [5, 3], keys, keys, diag, w):
            with pytest.raises(zk.ZkfheError, match=r"base_bits must be in \[1, 32\]"):
                call()
    for call in both(ctx, (1000, q, t, 19), np.zeros((1, 1000), np.uint64), np.zeros((1, 1000), np.uint64), [5], np.zeros((1, l, 1000), np.uint64),
                     np.zeros((1, l, 1000), np.uint64), np.zeros((1, 1000), np.uint64)):
        with pytest.raises(zk.ZkfheError, match="bfv params"):
            call()
    # n = 0, n_elems = 0 and NULL pointers, at the C boundary
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib, prm = ctx.lib, zk.BfvParamsC(*params)
    p, kp, dp = z.ctypes.data_as(u64p), keys.ctypes.data_as(u64p), diag.ctypes.data_as(u64p)
    out = np.zeros((2, n), dtype=np.uint64)
    op = out.ctypes.data_as(u64p)
    g = np.array([5, 3], dtype=np.uint64)
    gp = g.ctypes.data_as(u64p)
    good = [ctx.h, ctypes.byref(prm), 1, p, p, 2, gp, kp, kp, 16]
    for fn, tail in ((lib.zkfhe_bfv_apply_galois_many, [op, op]), (lib.zkfhe_bfv_linear_transform, [dp, op, op])):
        args = good + tail
        for pos in range(2, len(args)):
            if pos == 9:
                continue
            broken = list(args)
            broken[pos] = 0 if pos in (2, 5) else None
            assert fn(*broken) != 0, (fn.__name__, pos)
            assert "bad argument" in lib.zkfhe_last_error(ctx.h).decode()
    assert lib.zkfhe_bfv_linear_transform(*(good + [dp, op, op])) == 0   # the same arguments, whole


def test_range_refusal_comes_before_any_device_work(ctx):
    """N = 32768, T = 2013265921, Q just below 2^63, w = 32: 1 + 16 + 30 + 63 + 49 = 159 bits already at n_elems = 1"""
    import zk_fhe_amd as zk
    params, w = (32768, Q63, 2013265921, 19), 32
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    assert l == 2
    z = np.zeros((1, n), dtype=np.uint64)
    bad = np.full((1, n), q, dtype=np.uint64)   # would be refused by the passes over the inputs, which come later
    ctx.prof_enable(True)
    try:
        for count in (1, 3):
            keys = np.zeros((count, l, n), dtype=np.uint64)
            with pytest.raises(zk.ZkfheError, match="narrow base_bits, or split the element list"):
                ctx.bfv_linear_transform(params, bad, z, [5] * count, keys, keys, np.zeros((count, n), np.uint64), base_bits=w)
        for slot in range(5, 18):
            assert ctx.prof_read(slot)["launches"] == 0, slot
        # apply_galois_many never refuses on range: l N 2^w Q < 2^116
        keys = np.zeros((1, l, n), dtype=np.uint64)
        o0, o1 = ctx.bfv_apply_galois_many(params, z, z, [5], keys, keys, base_bits=w)
        assert not o0.any() and not o1.any()
        assert ctx.prof_read(zk.PROF_BFV_HOIST)["launches"] == 1 and ctx.prof_read(zk.PROF_BFV_LINEAR)["launches"] == 1
    finally:
        ctx.prof_enable(False)
    # T = 65537, w = 16 at the largest N is accepted
    p16 = (32768, Q63, 65537, 19)
    keys = np.zeros((1, relin_digits(Q63, 16), n), dtype=np.uint64)
    o0, o1 = ctx.bfv_linear_transform(p16, z, z, [5], keys, keys, z, base_bits=16)
    assert not o0.any() and not o1.any()


# ---- 7. the key rows of g = 1 ------------------------------------------------------------------------------------------------------

def test_identity_element_ignores_its_key_rows(ctx):
    params, w = B1024, 8
    n, q = params[0], params[1]
    rng = np.random.default_rng(27)
    sk = ctx.bfv_fhe_keypair(params, b"\x87" * 32)[0]
    elements = [1, galois_element(n, 2), 1]
    gk0, gk1 = keys_for(ctx, params, sk, elements, w)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    diag = plaintexts(rng, params, 3)
    want_many = ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w)
    want_lin = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    assert np.array_equal(want_many[0][0], c0) and np.array_equal(want_many[1][0], c1)
    assert np.array_equal(want_many[0][2], c0) and np.array_equal(want_many[1][2], c1)
    for k in (0, 2):
        gk0[k], gk1[k] = np.uint64(q), np.uint64(2 ** 64 - 1)
    got_many = ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w)
    got_lin = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    assert all(np.array_equal(a, b) for a, b in zip(want_many + want_lin, got_many + got_lin))
    # all-identity lists read no key at all
    o0, o1 = ctx.bfv_apply_galois_many(params, c0, c1, [1], gk0[:1], gk1[:1], base_bits=w)
    assert np.array_equal(o0[0], c0) and np.array_equal(o1[0], c1)
