"""The baby-step/giant-step linear transform on the GPU (bfv_linear.hip): zkfhe_bfv_linear_transform_bsgs bit for bit against the
restatement of tests/test_bfv_bsgs_host.py and against the composition through the existing GPU calls, across a ciphertext chunk and
a giant-step group, decrypted dense and banded matrix-vector products under a single key and under a three-party collective key,
every refusal, and the ignored key rows of g = 1.  Run on the MI355X box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

from tests.test_bfv_bsgs_host import ref_linear_transform_bsgs
from tests.test_bfv_eval_host import Q29, Q60, Q63, relin_digits
from tests.test_bfv_galois_host import galois_element

pytestmark = pytest.mark.gpu
A1024 = (1024, Q29, 12289, 19)
B1024 = (1024, Q60, 12289, 19)
B4096 = (4096, Q60, 65537, 19)
B32768 = (32768, Q60, 65537, 19)
CRS = b"\xc7" * 32
PARTIES = [bytes([0x58 + i]) * 32 for i in range(3)]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def residues(rng, params, count):
    return rng.integers(0, params[1], size=(count, params[0]), dtype=np.uint64)


def plaintexts(rng, params, shape):
    """random plaintexts over the whole range [0, T/2] and [Q - T/2, Q - 1]"""
    q, t = params[1], params[2]
    x = rng.integers(-(t // 2), t // 2 + 1, size=tuple(shape) + (params[0],)).astype(object)
    return (x % q).astype(np.uint64)


def keys_for(ctx, params, sk, elements, w, seed):
    """one key per distinct element, laid out per list entry (repeats share their rows)"""
    made = {g: ctx.bfv_galois_keygen(params, sk, g, seed=seed, base_bits=w) for g in set(elements)}
    return np.array([made[g][0] for g in elements]), np.array([made[g][1] for g in elements])


def grid(n):
    """3 x 3: g = 1 in both lists, a repeated element, the row swap and a swapped rotation"""
    return [1, galois_element(n, 3), galois_element(n, 3)], [galois_element(n, 40, True), 1, 2 * n - 1]


def chunk_rule(params, w, n_cts, n_baby, n_giant):
    """bsgs_chunks of bfv_linear.hip: (ciphertexts per chunk, giant steps per group)"""
    n, rows = params[0], relin_digits(params[1], w) + 1
    budget = max(8, (1 << 21) // n)
    cts = min(n_cts, max(1, budget // (max(rows, 2 * n_baby) + n_giant * rows)))
    if 4 < cts < n_cts:
        cts -= cts % 4   # whole tiles of 4 ciphertexts
    return cts, min(n_giant, max(1, budget // (cts * rows)))


# ---- 1. against the restatement --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", [(A1024, 4), (B4096, 16)])
def test_against_the_restatement(ctx, params, w):
    n = params[0]
    rng = np.random.default_rng(31)
    sk = ctx.bfv_fhe_keypair(params, b"\x90" * 32)[0]
    g_baby, g_giant = grid(n)
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\x91" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\x92" * 32)
    c0, c1 = residues(rng, params, 3), residues(rng, params, 3)
    diag = plaintexts(rng, params, (3, 3))
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w)
    assert o0.shape == o1.shape == (3, n)
    for j in (0, 2):
        r0, r1 = ref_linear_transform_bsgs(params, c0[j], c1[j], g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag)
        assert np.array_equal(o0[j], r0) and np.array_equal(o1[j], r1), j


# ---- 2. the composition through the existing calls -----------------------------------------------------------------------------

def compose(ctx, params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, w):
    acc = None
    for i, g in enumerate(g_giant):
        in0, in1 = ctx.bfv_linear_transform(params, c0, c1, g_baby, bk0, bk1, diag[i], base_bits=w)
        r0, r1 = ctx.bfv_apply_galois_many(params, in0, in1, [g], hk0[i:i + 1], hk1[i:i + 1], base_bits=w)
        acc = (r0[0], r1[0]) if acc is None else ctx.bfv_add(params, acc[0], acc[1], r0[0], r1[0])
    return acc


@pytest.mark.parametrize("params,w,count,small", [(B1024, 8, 5, False), (B4096, 16, 2, False), (B32768, 16, 1, True)])
def test_is_the_composition(ctx, params, w, count, small):
    n = params[0]
    rng = np.random.default_rng(32)
    sk = ctx.bfv_fhe_keypair(params, b"\x93" * 32)[0]
    g_baby, g_giant = grid(n)
    if small:   # n_giant x n_baby = 3 x 2 at the largest transform
        g_baby = g_baby[:2]
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\x94" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\x95" * 32)
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    diag = plaintexts(rng, params, (len(g_giant), len(g_baby)))
    want = compose(ctx, params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, w)
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w)
    assert np.array_equal(o0, want[0]) and np.array_equal(o1, want[1])


# ---- 3. chunk boundaries -----------------------------------------------------------------------------------------------------------

def test_across_a_ciphertext_chunk(ctx):
    """58 ciphertexts at N = 1024, w = 4 with the 3 x 3 grid: 9 hoisted rows per ciphertext and per giant step, so a ciphertext
    holds max(9, 6) + 3 * 9 = 36 polynomials and a chunk 2048 / 36 = 56 ciphertexts, with all 3 giant steps in one group"""
    params, w, count = A1024, 4, 58
    n = params[0]
    assert chunk_rule(params, w, count, 3, 3) == (56, 3)
    rng = np.random.default_rng(33)
    sk = ctx.bfv_fhe_keypair(params, b"\x96" * 32)[0]
    g_baby, g_giant = grid(n)
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\x97" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\x98" * 32)
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    diag = plaintexts(rng, params, (3, 3))
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w)
    for j in (0, 55, 56, 57):
        r0, r1 = ref_linear_transform_bsgs(params, c0[j], c1[j], g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag)
        assert np.array_equal(o0[j], r0) and np.array_equal(o1[j], r1), j


def test_across_a_giant_group(ctx):
    """One ciphertext at N = 1024, w = 1 (l = 29, 30 hoisted rows) with 2 baby and 70 giant steps: the ciphertext alone holds
    30 + 70 * 30 polynomials against the budget of 2048, so the chunk is 1 ciphertext and a group 2048 / 30 = 68 giant steps: steps
    0 to 67 and 68, 69.  Giant steps 0, 67, 68 and 69 have random diagonals and every other one zero diagonals.  A zero row has the
    inner ciphertext (0, 0), whose hoisted rotation is (0, 0), so the restatement of the four rows is the restatement of all 70."""
    params, w, n_giant = A1024, 1, 70
    n = params[0]
    assert chunk_rule(params, w, 1, 2, n_giant) == (1, 68)
    rng = np.random.default_rng(34)
    sk = ctx.bfv_fhe_keypair(params, b"\x99" * 32)[0]
    g_baby = [galois_element(n, 1), 1]
    cycle = [galois_element(n, 5), 2 * n - 1, 1, galois_element(n, 9, True)]
    g_giant = [cycle[i % 4] for i in range(n_giant)]
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\x9a" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\x9b" * 32)
    c0, c1 = residues(rng, params, 1), residues(rng, params, 1)
    live = [0, 67, 68, 69]
    diag = np.zeros((n_giant, 2, n), dtype=np.uint64)
    diag[live] = plaintexts(rng, params, (4, 2))
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w)
    r0, r1 = ref_linear_transform_bsgs(params, c0[0], c1[0], g_baby, bk0, bk1, [g_giant[i] for i in live], hk0[live], hk1[live], w, diag[live])
    assert np.array_equal(o0[0], r0) and np.array_equal(o1[0], r1)
    # and the two groups one at a time add up to the same
    a = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant[:68], hk0[:68], hk1[:68], diag[:68], base_bits=w)
    b = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant[68:], hk0[68:], hk1[68:], diag[68:], base_bits=w)
    s0, s1 = ctx.bfv_add(params, a[0], a[1], b[0], b[1])
    assert np.array_equal(o0, s0) and np.array_equal(o1, s1)


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


def encode_grid(ctx, params, d):
    return ctx.bfv_encode_slots(params, d.reshape(-1, params[0])).reshape(d.shape)


def test_dense_matrix_decrypts(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 8
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(35)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x9c" * 32)
    m = rng.integers(0, t, size=(n, n), dtype=np.int64)
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, m)
    assert len(g_baby) == 32 and len(g_giant) == 32 and sum(g != 1 for g in g_baby + g_giant) == 62   # 62 keys
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\x9d" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\x9e" * 32)
    v = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\x9f" * 32)
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, ct["c0"], ct["c1"], g_baby, bk0, bk1, g_giant, hk0, hk1, encode_grid(ctx, params, d), base_bits=w)
    noise, limit = int(ctx.bfv_noise(params, sk, o0, o1).max()), (q // t) // 2
    print("dense 1024 x 1024 product, w = %d, 62 keys: noise 2^%.1f, limit 2^%.1f" % (w, np.log2(max(noise, 1)), np.log2(limit)))
    got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, o0, o1))
    for j in range(2):
        assert np.array_equal(got[j], matvec(params, m, v[j])), j
    assert noise < limit


def test_banded_matrix_decrypts_as_the_flat_call(ctx):
    import zk_fhe_amd as zk
    params, w = B4096, 4
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(36)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\xa0" * 32)
    m = banded(rng, params, (0, 1, 2, 3, 70, 130), (0, 1, 65))
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, m, 64)
    assert g_baby == [galois_element(n, b) for b in (0, 1, 2, 3, 6)]
    assert g_giant == [galois_element(n, 0), galois_element(n, 64), galois_element(n, 128), 2 * n - 1, galois_element(n, 64, True)]
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\xa1" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\xa2" * 32)
    v = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\xa3" * 32)
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, ct["c0"], ct["c1"], g_baby, bk0, bk1, g_giant, hk0, hk1, encode_grid(ctx, params, d), base_bits=w)
    noise, limit = int(ctx.bfv_noise(params, sk, o0, o1).max()), (q // t) // 2
    print("banded product at N = 4096, w = %d, 5 + 5 elements: noise 2^%.1f, limit 2^%.1f" % (w, np.log2(max(noise, 1)), np.log2(limit)))
    got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, o0, o1))
    elements, fd = zk.bfv_matrix_diagonals(params, m)
    assert len(elements) == 9
    gk0, gk1 = keys_for(ctx, params, sk, elements, w, b"\xa4" * 32)
    f0, f1 = ctx.bfv_linear_transform(params, ct["c0"], ct["c1"], elements, gk0, gk1, ctx.bfv_encode_slots(params, fd), base_bits=w)
    flat = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, f0, f1))
    for j in range(2):
        assert np.array_equal(got[j], matvec(params, m, v[j])), j
    assert np.array_equal(got, flat)
    assert noise < limit


# ---- 5. under a collective key -------------------------------------------------------------------------------------------------

def test_banded_matrix_under_a_collective_key(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 8
    n, t = params[0], params[2]
    rng = np.random.default_rng(37)
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES]
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]
    m = banded(rng, params, (0, 1, 2, 5), (0, 3))
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, m, 2)
    assert len(g_baby) == 2 and len(g_giant) == 5   # 5 joint key generations (g = 1 twice) against 6 diagonals

    def joint(elements):
        l = relin_digits(params[1], w)
        k0, k1 = np.zeros((len(elements), l, n), dtype=np.uint64), np.zeros((len(elements), l, n), dtype=np.uint64)
        for i, g in enumerate(elements):
            if g == 1:
                continue   # never read
            shares = [ctx.bfv_galois_share(params, sk, CRS, ps, g, base_bits=w) for sk, ps in zip(sks, PARTIES)]
            k0[i], k1[i] = ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])), shares[0][1]
        return k0, k1

    bk0, bk1 = joint(g_baby)
    hk0, hk1 = joint(g_giant)
    v = rng.integers(0, t, size=(1, n), dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\xa5" * 32)
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, ct["c0"], ct["c1"], g_baby, bk0, bk1, g_giant, hk0, hk1, encode_grid(ctx, params, d), base_bits=w)
    shares = [ctx.bfv_decrypt_share(params, sk, o1, seed=bytes([0x79, i]) * 16, smudge_bound=1 << 20) for i, sk in enumerate(sks)]
    got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt_combine(params, o0, np.array(shares)))
    assert np.array_equal(got[0], matvec(params, m, v[0]))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import zk_fhe_amd as zk
    params = B1024
    n, q, t = params[0], params[1], params[2]
    l = relin_digits(q, 16)
    z = np.zeros((1, n), dtype=np.uint64)
    keys = np.zeros((2, l, n), dtype=np.uint64)
    diag = np.zeros((2, 2, n), dtype=np.uint64)

    def call(c0=z, c1=z, gb=(5, 3), bk0=keys, bk1=keys, gg=(25, 3), hk0=keys, hk1=keys, d=diag, w=16, prm=params):
        return ctx.bfv_linear_transform_bsgs(prm, c0, c1, list(gb), bk0, bk1, list(gg), hk0, hk1, d, base_bits=w)

    o0, o1 = call()
    assert not o0.any() and not o1.any()
    for g in (0, 4, 2 * n, 2 * n + 1):
        for kw in ({"gb": (5, g)}, {"gg": (g, 5)}):
            with pytest.raises(zk.ZkfheError, match="odd and below 2N"):
                call(**kw)
    big = z.copy()
    big[0, 3] = q
    for kw in ({"c0": big}, {"c1": big}):
        with pytest.raises(zk.ZkfheError, match="ciphertext coefficient is not below Q"):
            call(**kw)
    bad = keys.copy()
    bad[1, 1, 2] = q
    for name in ("bk0", "bk1", "hk0", "hk1"):
        with pytest.raises(zk.ZkfheError, match="Galois-key coefficient is not below Q"):
            call(**{name: bad})
    for value in (t // 2 + 1, q - t // 2 - 1, q):
        bd = diag.copy()
        bd[1, 0, 7] = value
        with pytest.raises(zk.ZkfheError, match="a diagonal coefficient is outside"):
            call(d=bd)
    for w in (0, 33):
        with pytest.raises(zk.ZkfheError, match=r"base_bits must be in \[1, 32\]"):
            call(w=w)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        z1000, k1000 = np.zeros((1, 1000), np.uint64), np.zeros((2, l, 1000), np.uint64)
        call(c0=z1000, c1=z1000, bk0=k1000, bk1=k1000, hk0=k1000, hk1=k1000, d=np.zeros((2, 2, 1000), np.uint64), prm=(1000, q, t, 19))
    # NULL pointers, zero counts and counts of 2^20 at the C boundary
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib, prm = ctx.lib, zk.BfvParamsC(*params)
    fn = lib.zkfhe_bfv_linear_transform_bsgs
    p, kp, dp = z.ctypes.data_as(u64p), keys.ctypes.data_as(u64p), diag.ctypes.data_as(u64p)
    out = np.zeros((2, n), dtype=np.uint64)
    op = out.ctypes.data_as(u64p)
    g = np.array([5, 3], dtype=np.uint64)
    gp = g.ctypes.data_as(u64p)
    good = [ctx.h, ctypes.byref(prm), 1, p, p, 2, gp, kp, kp, 2, gp, kp, kp, 16, dp, op, op]
    for pos in range(2, len(good)):
        if pos == 13:
            continue
        broken = list(good)
        broken[pos] = 0 if pos in (2, 5, 9) else None
        assert fn(*broken) != 0, pos
        assert "bad argument" in lib.zkfhe_last_error(ctx.h).decode()
    for pos in (5, 9):   # the count is refused before the list is read
        broken = list(good)
        broken[pos] = 1 << 20
        assert fn(*broken) != 0, pos
        assert "more than 2^20 Galois elements" in lib.zkfhe_last_error(ctx.h).decode()
    assert fn(*good) == 0   # the same arguments, whole


def test_range_refusal_comes_before_any_device_work(ctx):
    """N = 32768, T = 2013265921, Q just below 2^63, w = 32: 1 + 16 + 30 + 63 + 49 = 159 bits already at n_baby = 1"""
    import zk_fhe_amd as zk
    params, w = (32768, Q63, 2013265921, 19), 32
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    assert l == 2
    z = np.zeros((1, n), dtype=np.uint64)
    bad = np.full((1, n), q, dtype=np.uint64)   # would be refused by the passes over the inputs, which come later
    ctx.prof_enable(True)
    try:
        for n_baby, n_giant in ((1, 1), (3, 2)):
            bk, hk = np.zeros((n_baby, l, n), dtype=np.uint64), np.zeros((n_giant, l, n), dtype=np.uint64)
            with pytest.raises(zk.ZkfheError, match="narrow base_bits, or split the element list"):
                ctx.bfv_linear_transform_bsgs(params, bad, z, [5] * n_baby, bk, bk, [25] * n_giant, hk, hk, np.zeros((n_giant, n_baby, n), np.uint64), base_bits=w)
        for slot in range(5, 20):
            assert ctx.prof_read(slot)["launches"] == 0, slot
    finally:
        ctx.prof_enable(False)
    # T = 65537, w = 16 at the largest N is accepted, and its own kernels count in their slots
    p16 = (32768, Q63, 65537, 19)
    keys = np.zeros((1, relin_digits(Q63, 16), n), dtype=np.uint64)
    ctx.prof_enable(True)
    try:
        o0, o1 = ctx.bfv_linear_transform_bsgs(p16, z, z, [5], keys, keys, [25], keys, keys, np.zeros((1, 1, n), np.uint64), base_bits=16)
        assert not o0.any() and not o1.any()
        assert ctx.prof_read(zk.PROF_BFV_BSGS_INNER)["launches"] == 1 and ctx.prof_read(zk.PROF_BFV_BSGS_GIANT)["launches"] == 1
        assert ctx.prof_read(zk.PROF_BFV_HOIST)["launches"] == 2 and ctx.prof_read(zk.PROF_BFV_LINEAR)["launches"] == 1
    finally:
        ctx.prof_enable(False)


# ---- 7. the key rows of g = 1 ------------------------------------------------------------------------------------------------------

def test_identity_elements_ignore_their_key_rows(ctx):
    params, w = B1024, 8
    n, q = params[0], params[1]
    rng = np.random.default_rng(38)
    sk = ctx.bfv_fhe_keypair(params, b"\xa6" * 32)[0]
    g_baby, g_giant = [1, galois_element(n, 2), 1], [galois_element(n, 4), 1]
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\xa7" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\xa8" * 32)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    diag = plaintexts(rng, params, (2, 3))
    want = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w)
    for k in (0, 2):
        bk0[k], bk1[k] = np.uint64(q), np.uint64(2 ** 64 - 1)
    hk0[1], hk1[1] = np.uint64(2 ** 64 - 1), np.uint64(q)
    got = ctx.bfv_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    # all-identity lists read no key at all: the product with one plaintext
    one = ctx.bfv_linear_transform_bsgs(params, c0, c1, [1], bk0[:1], bk1[:1], [1], hk0[1:], hk1[1:], diag[:1, :1], base_bits=w)
    p0, p1 = ctx.bfv_mul_plain(params, c0, c1, diag[0, 0])
    assert np.array_equal(one[0], p0) and np.array_equal(one[1], p1)
