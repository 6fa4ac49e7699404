"""BFV evaluation on the GPU (bfv_eval.hip): ciphertext products bit for bit against their definition in zkfhe.h (the Kronecker
oracle of tests/test_bfv_eval_host.py), the CRT bound at its edge, the relinearization key restated from zk.chacha20_block,
decryption after products, sums, additions and plaintext operations, the noise query, and argument errors.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60, Q63, centred, circ, deg, kron_negacyclic, ref_mul, relin_digits
from tests.test_gpu_bfv_encrypt import error, negacyclic, random_m, uniform

pytestmark = pytest.mark.gpu
K13 = (1024, Q29, 7, 19)   # the k = 13 parameters (examples/bfv.rs)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def random_residues(rng, shape, q):
    return rng.integers(0, q, size=shape, dtype=np.uint64)


def plain_product(m1, m2, params):
    """m1 m2 mod (x^N + 1, T), centred like the decryption, as residues mod Q (CircuitInput order)"""
    n, q, t = params[0], params[1], params[2]
    x = kron_negacyclic([(centred(deg(m1), q), centred(deg(m2), q))], n)
    r = [v % t for v in x]
    return circ([v - t if v > t // 2 else v for v in r], q)


def host_noise(params, sk, c0, c1):
    """zkfhe_bfv_noise restated: max |[c0 + c1 s - floor(Q/T) m]_Q| with m the decryption of inputs.decrypt"""
    n, q, t = params[0], params[1], params[2]
    out = []
    for j in range(c0.shape[0]):
        v = (c0[j].astype(object) + negacyclic(c1[j], sk, q).astype(object)) % q
        worst = 0
        for x in v:
            x = int(x)
            xc = x - q if x > q // 2 else x
            m = (2 * t * xc + q) // (2 * q) % t
            m = m - t if m > t // 2 else m
            e = (x - (q // t) * m) % q
            worst = max(worst, q - e if e > q // 2 else e)
        out.append(worst)
    return out


def fresh(ctx, params, count, key_seed, enc_seed, rng):
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, key_seed)
    m = random_m(rng, (count, params[0]), params[1], params[2])
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, enc_seed)
    return sk, m, ct["c0"], ct["c1"]


# ---- 1. products bit for bit ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,w", [(1024, Q29, 7, 8), (4096, Q60, 65537, 16), (16384, Q60, 65537, 32)])
def test_mul_bit_exact(ctx, n, q, t, w):
    params = (n, q, t, 19)
    rng = np.random.default_rng(n + w)
    sk, m, c0, c1 = fresh(ctx, params, 2, bytes([w]) * 32, bytes([w + 1]) * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, bytes([w + 2]) * 32, base_bits=w)
    assert rlk0.shape == (relin_digits(q, w), n)
    # pair 0: two encryptions; pair 1: arbitrary residues
    a0 = np.stack([c0[0], random_residues(rng, n, q)])
    a1 = np.stack([c1[0], random_residues(rng, n, q)])
    b0 = np.stack([c0[1], random_residues(rng, n, q)])
    b1 = np.stack([c1[1], random_residues(rng, n, q)])
    out0, out1 = ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)
    for j in range(2):
        want0, want1 = ref_mul(params, a0[j], a1[j], b0[j], b1[j], rlk0, rlk1, w)
        assert np.array_equal(out0[j], want0), j
        assert np.array_equal(out1[j], want1), j
    if t == 7:
        assert np.array_equal(ctx.bfv_decrypt(params, sk, out0[:1], out1[:1])[0], plain_product(m[0], m[1], params))


def test_mul_crt_bound_at_the_edge(ctx):
    n, q, w = 32768, Q63, 32
    params = (n, q, q - 2, 1)   # T near Q
    h = q // 2
    l = relin_digits(q, w)
    assert l == 2
    # rlk0 = (1, 2^32) as constant polynomials: out0 = c^0 + d_0 + 2^32 d_1 = c^0 + c^2 mod Q
    one = np.zeros(n, dtype=np.uint64)
    one[n - 1] = 1
    rlk0 = np.stack([one, one << np.uint64(32)])
    # pair 0, every coefficient +-floor(Q/2) with one sign per polynomial: x_k = s v^2 (2k + 2 - N), |x1| = 2 N v^2 at k = N - 1
    signs = (1, -1, -1, 1)   # a0, a1, b0, b1: x0 and x2 negative, x1 = 2 v^2 (2k + 2 - N)
    const = [np.full(n, h if s > 0 else q - h, dtype=np.uint64) for s in signs]
    full_q = np.full((l, n), q - 1, dtype=np.uint64)   # rlk1_i = all Q - 1: the largest relinearization sum
    out0, out1 = ctx.bfv_mul(params, *[c[None] for c in const], rlk0, full_q, base_bits=w)
    sa0, sa1, sb0, sb1 = signs
    t = params[2]
    rnd = lambda x: (2 * t * x + q) // (2 * q) % q  # noqa: E731
    x0 = [sa0 * sb0 * h * h * (2 * k + 2 - n) for k in range(n)]
    x1 = [(sa0 * sb1 + sa1 * sb0) * h * h * (2 * k + 2 - n) for k in range(n)]
    x2 = [sa1 * sb1 * h * h * (2 * k + 2 - n) for k in range(n)]
    assert max(abs(x) for x in x1) == 2 * n * h * h and (2 * n * h * h).bit_length() == 140
    c0h, c1h, c2h = [rnd(x) for x in x0], [rnd(x) for x in x1], [rnd(x) for x in x2]
    assert np.array_equal(out0[0], circ([a + b for a, b in zip(c0h, c2h)], q))
    # sum_i d_i * (Q - 1, ..., Q - 1): coefficient k = (Q - 1) (prefix_k - suffix_k) of s = d_0 + d_1
    s = [(c & 0xFFFFFFFF) + (c >> 32) for c in c2h]
    pre, acc = [], 0
    for v in s:
        acc += v
        pre.append(acc)
    relin1 = [(q - 1) * (pre[k] - (acc - pre[k])) for k in range(n)]
    assert np.array_equal(out1[0], circ([a + b for a, b in zip(c1h, relin1)], q))
    # pair 1: random signs at +-floor(Q/2), 64 positions by the schoolbook sum; rlk1 = 0 leaves out1 = c^1
    rng = np.random.default_rng(5)
    polys = [np.where(rng.integers(0, 2, n) == 1, np.uint64(h), np.uint64(q - h)).astype(np.uint64) for _ in range(4)]
    out0, out1 = ctx.bfv_mul(params, *[p[None] for p in polys], rlk0, np.zeros((l, n), dtype=np.uint64), base_bits=w)
    A0, A1, B0, B1 = (np.array(centred(deg(p), q), dtype=object) for p in polys)

    def coeff(a, b, k):   # schoolbook, exact on Python integers
        return np.dot(a[:k + 1], b[k::-1]) - (np.dot(a[k + 1:], b[n - 1:k:-1]) if k < n - 1 else 0)

    for k in sorted(set(rng.integers(0, n, 62).tolist()) | {0, n - 1}):
        pos = n - 1 - k
        c0k, c2k = rnd(coeff(A0, B0, k)), rnd(coeff(A1, B1, k))
        c1k = rnd(coeff(A0, B1, k) + coeff(A1, B0, k))
        assert int(out0[0][pos]) == (c0k + c2k) % q, k
        assert int(out1[0][pos]) == c1k, k


# ---- 2. the relinearization key ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,w", [(1024, Q29, 7, 8), (4096, Q60, 65537, 16)])
def test_relin_key_restated(ctx, n, q, t, w):
    params = (n, q, t, 19)
    sk, _, _ = ctx.bfv_fhe_keypair(params, b"\x21" * 32)
    seed = bytes(range(40, 72))
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed, base_bits=w)
    l = relin_digits(q, w)
    assert rlk0.shape == rlk1.shape == (l, n) and rlk0.dtype == np.uint64
    s2 = circ(kron_negacyclic([(centred(deg(sk), q), centred(deg(sk), q))], n), q).astype(object)
    for i in range(l):
        a = uniform(seed, 7, i, n, q)
        e = error(seed, 8, i, n, q, 19)
        assert np.array_equal(rlk1[i], a), i
        want = ((s2 * (1 << (i * w))) - negacyclic(a, sk, q).astype(object) - e.astype(object)) % q
        assert np.array_equal(rlk0[i].astype(object), want), i
    again = ctx.bfv_relin_keygen(params, sk, seed, base_bits=w)
    assert np.array_equal(again[0], rlk0) and np.array_equal(again[1], rlk1)
    other = ctx.bfv_relin_keygen(params, sk, b"\x22" * 32, base_bits=w)
    assert not np.array_equal(other[1], rlk1)


# ---- 3. decryption after products -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,w", [(1024, Q29, 7, 8), (4096, Q60, 7, 16)])
def test_decrypt_after_mul(ctx, n, q, t, w):
    params = (n, q, t, 19)
    rng = np.random.default_rng(q % 1000 + w)
    sk, m, c0, c1 = fresh(ctx, params, 6, bytes([w + 3]) * 32, bytes([w + 4]) * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, bytes([w + 5]) * 32, base_bits=w)
    p0, p1 = ctx.bfv_mul(params, c0[:3], c1[:3], c0[3:], c1[3:], rlk0, rlk1, base_bits=w)
    dec = ctx.bfv_decrypt(params, sk, p0, p1)
    for j in range(3):
        assert np.array_equal(dec[j], plain_product(m[j], m[3 + j], params)), j
    noise = ctx.bfv_noise(params, sk, p0, p1)
    assert (noise < (q // t) // 2).all()
    if n == 4096:   # depth 2: (m0 m3) m1
        d0, d1 = ctx.bfv_mul(params, p0[:1], p1[:1], c0[1:2], c1[1:2], rlk0, rlk1, base_bits=w)
        want = plain_product(plain_product(m[0], m[3], params), m[1], params)
        assert np.array_equal(ctx.bfv_decrypt(params, sk, d0, d1)[0], want)
        assert ctx.bfv_noise(params, sk, d0, d1)[0] > noise[0]


# ---- 4. sums, additions, plaintext operations ----------------------------------------------------------------------------------

def test_sum_of_1000(ctx):
    params = K13
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(1000)
    sk, m, c0, c1 = fresh(ctx, params, 1000, b"\x31" * 32, b"\x32" * 32, rng)
    s0, s1 = ctx.bfv_sum(params, c0, c1)
    assert s0.shape == (n,) and s1.shape == (n,)
    assert np.array_equal(s0.astype(object), c0.astype(object).sum(axis=0) % q)
    assert np.array_equal(s1.astype(object), c1.astype(object).sum(axis=0) % q)
    msum = np.array(centred(m.reshape(-1), q), dtype=object).reshape(m.shape).sum(axis=0) % t
    want = np.array([int(v - t) % q if v > t // 2 else int(v) for v in msum], dtype=np.uint64)
    assert np.array_equal(ctx.bfv_decrypt(params, sk, s0, s1)[0], want)
    one0, one1 = ctx.bfv_sum(params, c0[:1], c1[:1])
    assert np.array_equal(one0, c0[0]) and np.array_equal(one1, c1[0])


def test_add_subtract_add_plain_mul_plain(ctx):
    params = (4096, Q60, 7, 19)
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(4)
    sk, m, c0, c1 = fresh(ctx, params, 6, b"\x41" * 32, b"\x42" * 32, rng)
    add0, add1 = ctx.bfv_add(params, c0[:3], c1[:3], c0[3:], c1[3:])
    sub0, sub1 = ctx.bfv_add(params, c0[:3], c1[:3], c0[3:], c1[3:], subtract=True)
    A0, A1, B0, B1 = (x.astype(object) for x in (c0[:3], c1[:3], c0[3:], c1[3:]))
    assert np.array_equal(add0.astype(object), (A0 + B0) % q) and np.array_equal(add1.astype(object), (A1 + B1) % q)
    assert np.array_equal(sub0.astype(object), (A0 - B0) % q) and np.array_equal(sub1.astype(object), (A1 - B1) % q)
    mc = np.array(centred(m.reshape(-1), q), dtype=object).reshape(m.shape)

    def as_plain(x):
        x = x % t
        return np.array([int(v - t) % q if v > t // 2 else int(v) for v in x.reshape(-1)], dtype=np.uint64).reshape(x.shape)

    assert np.array_equal(ctx.bfv_decrypt(params, sk, add0, add1), as_plain(mc[:3] + mc[3:]))
    assert np.array_equal(ctx.bfv_decrypt(params, sk, sub0, sub1), as_plain(mc[:3] - mc[3:]))
    # plaintext operands: one shared, or one per ciphertext
    pm = random_m(rng, (3, n), q, t)
    delta = q // t
    for shared in (True, False):
        mm = pm[0] if shared else pm
        ap0, ap1 = ctx.bfv_add_plain(params, c0[:3], c1[:3], mm)
        mp0, mp1 = ctx.bfv_mul_plain(params, c0[:3], c1[:3], mm)
        assert np.array_equal(ap1, c1[:3])
        for j in range(3):
            mj = pm[0] if shared else pm[j]
            md = np.array([(delta * v) % q for v in centred(mj, q)], dtype=object)
            assert np.array_equal(ap0[j].astype(object), (c0[j].astype(object) + md) % q), j
            mcen = centred(deg(mj), q)
            assert np.array_equal(mp0[j], circ(kron_negacyclic([(centred(deg(c0[j]), q), mcen)], n), q)), j
            assert np.array_equal(mp1[j], circ(kron_negacyclic([(centred(deg(c1[j]), q), mcen)], n), q)), j
            assert np.array_equal(ctx.bfv_decrypt(params, sk, ap0[j], ap1[j])[0], as_plain(mc[j] + np.array(centred(mj, q), dtype=object))), j
            assert np.array_equal(ctx.bfv_decrypt(params, sk, mp0[j], mp1[j])[0], plain_product(m[j], mj, params)), j


# ---- 5. the noise query -----------------------------------------------------------------------------------------------------

def test_noise_matches_host(ctx):
    params = K13
    q, t, w = params[1], params[2], 8
    rng = np.random.default_rng(9)
    sk, m, c0, c1 = fresh(ctx, params, 4, b"\x51" * 32, b"\x52" * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, b"\x53" * 32, base_bits=w)
    s0, s1 = ctx.bfv_sum(params, c0, c1)
    p0, p1 = ctx.bfv_mul(params, c0[:2], c1[:2], c0[2:], c1[2:], rlk0, rlk1, base_bits=w)
    for x0, x1 in ((c0, c1), (s0[None], s1[None]), (p0, p1)):
        got = ctx.bfv_noise(params, sk, x0, x1)
        assert got.dtype == np.uint64 and got.shape == (x0.shape[0],)
        assert [int(v) for v in got] == host_noise(params, sk, x0, x1)
    fresh_noise = ctx.bfv_noise(params, sk, c0, c1)
    assert (fresh_noise <= 19 * 1024 * 3).all()   # |e0 + e1 s - u e| stays far below delta / 2
    assert ctx.bfv_noise(params, sk, p0, p1).max() > fresh_noise.max()


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors(ctx):
    import zk_fhe_amd as zk
    params = K13
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(6)
    sk, m, c0, c1 = fresh(ctx, params, 2, b"\x61" * 32, b"\x62" * 32, rng)
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, b"\x63" * 32, base_bits=8)
    bad = c0.copy()
    bad[1, 7] = q
    with pytest.raises(zk.ZkfheError, match="bfv_add: a ciphertext coefficient is not below Q"):
        ctx.bfv_add(params, bad, c1, c0, c1)
    with pytest.raises(zk.ZkfheError, match="bfv_sum: a ciphertext coefficient is not below Q"):
        ctx.bfv_sum(params, c0, bad)
    with pytest.raises(zk.ZkfheError, match="bfv_add_plain: a ciphertext coefficient is not below Q"):
        ctx.bfv_add_plain(params, bad, c1, m[0])
    with pytest.raises(zk.ZkfheError, match="bfv_mul_plain: a ciphertext coefficient is not below Q"):
        ctx.bfv_mul_plain(params, c0, bad, m[0])
    with pytest.raises(zk.ZkfheError, match="bfv_mul: a ciphertext coefficient is not below Q"):
        ctx.bfv_mul(params, c0, c1, c0, bad, rlk0, rlk1, base_bits=8)
    with pytest.raises(zk.ZkfheError, match="bfv_noise: a ciphertext coefficient is not below Q"):
        ctx.bfv_noise(params, sk, bad, c1)
    bad_rlk = rlk1.copy()
    bad_rlk[0, 0] = 1 << 62
    with pytest.raises(zk.ZkfheError, match="bfv_mul: a relinearization-key coefficient is not below Q"):
        ctx.bfv_mul(params, c0, c1, c0, c1, rlk0, bad_rlk, base_bits=8)
    bad_m = m[0].copy()
    bad_m[3] = t // 2 + 1
    with pytest.raises(zk.ZkfheError, match="bfv_add_plain: a plaintext coefficient is outside"):
        ctx.bfv_add_plain(params, c0, c1, bad_m)
    with pytest.raises(zk.ZkfheError, match="bfv_mul_plain: a plaintext coefficient is outside"):
        ctx.bfv_mul_plain(params, c0, c1, bad_m)
    bad_sk = sk.copy()
    bad_sk[5] = 2
    with pytest.raises(zk.ZkfheError, match="bfv_relin_keygen: a secret-key coefficient is not in"):
        ctx.bfv_relin_keygen(params, bad_sk, b"\x64" * 32, base_bits=8)
    with pytest.raises(zk.ZkfheError, match="bfv_noise: a secret-key coefficient is not in"):
        ctx.bfv_noise(params, bad_sk, c0, c1)
    for w in (0, 33):
        with pytest.raises(zk.ZkfheError, match=r"bfv_relin_keygen: base_bits must be in \[1, 32\]"):
            ctx.bfv_relin_keygen(params, sk, b"\x64" * 32, base_bits=w)
        with pytest.raises(zk.ZkfheError, match=r"bfv_mul: base_bits must be in \[1, 32\]"):
            ctx.bfv_mul(params, c0, c1, c0, c1, rlk0, rlk1, base_bits=w)
    # shapes
    with pytest.raises(ValueError, match="same shape"):
        ctx.bfv_add(params, c0, c1, c0[:1], c1[:1])
    with pytest.raises(ValueError, match="rlk0 and rlk1"):
        ctx.bfv_mul(params, c0, c1, c0, c1, rlk0[:-1], rlk1[:-1], base_bits=8)
    with pytest.raises(ValueError, match="rlk0 and rlk1"):
        ctx.bfv_mul(params, c0, c1, c0, c1, rlk0, rlk1, base_bits=16)
    with pytest.raises(ValueError, match="one per ciphertext"):
        ctx.bfv_mul_plain(params, c0, c1, np.zeros((3, n), dtype=np.uint64))
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        ctx.bfv_add(params[:2] + (q, 19), c0, c1, c0, c1)   # T >= Q
    # the context still works
    a0, a1 = ctx.bfv_add(params, c0, c1, c0, c1)
    assert np.array_equal(ctx.bfv_decrypt(params, sk, *ctx.bfv_add(params, a0, a1, c0, c1, subtract=True)), m)
