"""Host side of threshold BFV (no GPU): the declarations and exports of the new entry points, and a pure-Python restatement of the
protocol of zkfhe.h (collective key, two-round relinearization key, decryption shares and their combination) from zk.chacha20_block,
zk.bfv_error_cdt and the Kronecker oracle of tests/test_bfv_eval_host.py.  At N = 16 it checks the relinearization identity exactly
and that combining the shares is decryption under s = sum_i s_i.  tests/test_gpu_bfv_threshold.py imports these restatements."""
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, centred, circ, deg, kron_negacyclic, relin_digits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_keygen_share", "zkfhe_bfv_share_aggregate", "zkfhe_bfv_relin_share1", "zkfhe_bfv_relin_share2",
               "zkfhe_bfv_decrypt_share", "zkfhe_bfv_decrypt_combine"]
METHODS = ["bfv_keygen_share", "bfv_share_aggregate", "bfv_relin_share1", "bfv_relin_share2", "bfv_decrypt_share", "bfv_decrypt_combine"]


# ---- samplers (ChaCha20 layout of zkfhe_bfv_encrypt: array position p reads word p) ------------------------------------------

def words(seed, domain, index, n_words):
    out = []
    for blk in range((n_words + 7) // 8):
        b = zk.chacha20_block(seed, [blk, domain, index & 0xFFFFFFFF, index >> 32])
        out += [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(8)]
    return out[:n_words]


def ternary(seed, domain, index, n, q):
    return np.array([((w * 3 >> 64) - 1) % q for w in words(seed, domain, index, n)], dtype=np.uint64)


def uniform_ints(seed, domain, index, n, m):
    """(x M) >> 128 with x = w[2p] + 2^64 w[2p + 1]: integers in [0, M)"""
    w = words(seed, domain, index, 2 * n)
    return [((w[2 * p] | w[2 * p + 1] << 64) * m) >> 128 for p in range(n)]


def uniform(seed, domain, index, n, q):
    return np.array(uniform_ints(seed, domain, index, n, q), dtype=np.uint64)


def error(seed, domain, index, n, q, b):
    cdt = zk.bfv_error_cdt((8, q, 2, b))
    w = np.array(words(seed, domain, index, n), dtype=np.uint64)
    x = np.searchsorted(cdt, w, side="right").astype(np.int64) - b   # #{i : T_i <= w} - B
    return np.array([int(v) % q for v in x], dtype=np.uint64)


def smudge(seed, index, n, q, bound):
    """the smudging noise of a decryption share: uniform mod 2E + 1 minus E (domain 9), as residues mod Q"""
    return np.array([(x - bound) % q for x in uniform_ints(seed, 9, index, n, 2 * bound + 1)], dtype=np.uint64)


# ---- ring arithmetic on CircuitInput-order residue arrays ----------------------------------------------------------------------

def ring_mul(a, b, q):
    """a b mod (x^N + 1, Q), both read centred (exact over Z first)"""
    return circ(kron_negacyclic([(centred(deg(a), q), centred(deg(b), q))], len(a)), q)


def add(*vs, q):
    return np.array([sum(int(x) for x in col) % q for col in zip(*vs)], dtype=np.uint64)


def neg(v, q):
    return np.array([(q - int(x)) % q for x in v], dtype=np.uint64)


def decrypt_round(v, q, t):
    """EPI_DECRYPT of zkfhe_bfv_decrypt on the residue v = [c0 + c1 s]_Q"""
    m = (2 * t * v + q) // (2 * q)
    m = 0 if m == t else m
    return q - (t - m) if m > t // 2 else m


# ---- the protocol, restated from zkfhe.h -------------------------------------------------------------------------------------

def ref_keygen_share(params, crs_seed, party_seed):
    n, q, b = params[0], params[1], params[3]
    s = ternary(party_seed, 4, 0, n, q)
    a = uniform(crs_seed, 5, 0, n, q)
    e = error(party_seed, 6, 0, n, q, b)
    return s, neg(add(ring_mul(a, s, q), e, q=q), q), a


def ref_aggregate(params, shares):
    q = params[1]
    shares = np.asarray(shares, dtype=np.uint64)
    return (shares.astype(object).sum(axis=0) % q).astype(np.uint64)


def ref_relin_share1(params, s, crs_seed, party_seed, w):
    n, q, b = params[0], params[1], params[3]
    l = relin_digits(q, w)
    u = ternary(party_seed, 10, 0, n, q)
    h0, h1 = [], []
    for j in range(l):
        a = uniform(crs_seed, 7, j, n, q)
        e0, e1 = error(party_seed, 11, j, n, q, b), error(party_seed, 12, j, n, q, b)
        gadget = np.array([(int(x) if int(x) < 2 else int(x) - q) * (1 << (j * w)) % q for x in s], dtype=np.uint64)
        h0.append(add(neg(ring_mul(u, a, q), q), gadget, e0, q=q))
        h1.append(add(ring_mul(s, a, q), e1, q=q))
    return np.array(h0), np.array(h1)


def ref_relin_share2(params, s, party_seed, h0, h1, w):
    n, q, b = params[0], params[1], params[3]
    u = ternary(party_seed, 10, 0, n, q)
    u_minus_s = add(u, neg(s, q), q=q)
    return np.array([add(ring_mul(s, h0[j], q), ring_mul(u_minus_s, h1[j], q), error(party_seed, 13, j, n, q, b), q=q)
                     for j in range(relin_digits(q, w))])


def ref_decrypt_share(params, s, c1, seed, first_index, bound):
    n, q = params[0], params[1]
    c1 = np.asarray(c1, dtype=np.uint64).reshape(-1, n)
    return np.array([add(ring_mul(c1[j], s, q), smudge(seed, first_index + j, n, q, bound), q=q) for j in range(c1.shape[0])])


def ref_decrypt_combine(params, c0, d):
    n, q, t = params[0], params[1], params[2]
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1, n)
    d = np.asarray(d, dtype=np.uint64).reshape(-1, c0.shape[0], n)
    v = (c0.astype(object) + d.astype(object).sum(axis=0)) % q
    return np.array([[decrypt_round(int(x), q, t) for x in row] for row in v], dtype=np.uint64)


def collective_secret(params, sks):
    """s = sum_i s_i as residues mod Q (not ternary)"""
    return ref_aggregate(params, sks)


def ref_decrypt(params, s, c0, c1):
    """decryption under any s (the collective one included): the rounding of zkfhe_bfv_decrypt on [c0 + c1 s]_Q"""
    n, q, t = params[0], params[1], params[2]
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1, n)
    c1 = np.asarray(c1, dtype=np.uint64).reshape(-1, n)
    out = []
    for j in range(c0.shape[0]):
        v = add(c0[j], ring_mul(c1[j], s, q), q=q)
        out.append([decrypt_round(int(x), q, t) for x in v])
    return np.array(out, dtype=np.uint64)


def ref_noise(params, s, c0, c1, m):
    """max |[c0 + c1 s - floor(Q/T) m]_Q| (centred) over every coefficient, for the expected plaintext m"""
    n, q, t = params[0], params[1], params[2]
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1, n)
    c1 = np.asarray(c1, dtype=np.uint64).reshape(-1, n)
    m = np.asarray(m, dtype=np.uint64).reshape(-1, n)
    worst = 0
    for j in range(c0.shape[0]):
        v = add(c0[j], ring_mul(c1[j], s, q), q=q)
        for x, mv in zip(v, m[j]):
            mc = int(mv) - q if int(mv) > q // 2 else int(mv)
            e = (int(x) - (q // t) * mc) % q
            worst = max(worst, q - e if e > q // 2 else e)
    return worst


def relin_residual(params, rlk0, rlk1, s, w):
    """rlk0[j] + rlk1[j] s - 2^(j w) s^2 mod Q, per row"""
    q = params[1]
    s2 = ring_mul(s, s, q)
    return np.array([add(rlk0[j], ring_mul(rlk1[j], s, q), neg(np.array([int(x) * (1 << (j * w)) % q for x in s2], dtype=np.uint64), q), q=q)
                     for j in range(rlk0.shape[0])])


def relin_noise(params, sks, party_seeds, w):
    """s e0_j + u e1_j + e2_j mod Q per row, with the sums over the parties: what relin_residual must equal"""
    n, q, b = params[0], params[1], params[3]
    s = collective_secret(params, sks)
    u = ref_aggregate(params, [ternary(ps, 10, 0, n, q) for ps in party_seeds])
    out = []
    for j in range(relin_digits(q, w)):
        e0, e1, e2 = (ref_aggregate(params, [error(ps, dom, j, n, q, b) for ps in party_seeds]) for dom in (11, 12, 13))
        out.append(add(ring_mul(s, e0, q), ring_mul(u, e1, q), e2, q=q))
    return np.array(out)


def ref_collective_keys(params, crs_seed, party_seeds, w):
    """the whole key ceremony restated: (sks, pk0, pk1, rlk0, rlk1)"""
    keys = [ref_keygen_share(params, crs_seed, ps) for ps in party_seeds]
    sks = [k[0] for k in keys]
    pk0, pk1 = ref_aggregate(params, [k[1] for k in keys]), keys[0][2]
    r1 = [ref_relin_share1(params, s, crs_seed, ps, w) for s, ps in zip(sks, party_seeds)]
    h0, h1 = ref_aggregate(params, [x[0] for x in r1]), ref_aggregate(params, [x[1] for x in r1])
    rlk0 = ref_aggregate(params, [ref_relin_share2(params, s, ps, h0, h1, w) for s, ps in zip(sks, party_seeds)])
    return sks, pk0, pk1, rlk0, h1


def ref_encrypt(params, pk0, pk1, m, seed, index):
    """zkfhe_bfv_encrypt of one message restated (domains 1, 2, 3)"""
    n, q, t, b = params
    u = ternary(seed, 1, index, n, q)
    mc = np.array([(int(x) - q if int(x) > q // 2 else int(x)) * (q // t) % q for x in m], dtype=np.uint64)
    c0 = add(ring_mul(pk0, u, q), mc, error(seed, 2, index, n, q, b), q=q)
    c1 = add(ring_mul(pk1, u, q), error(seed, 3, index, n, q, b), q=q)
    return c0, c1


# ---- tests -------------------------------------------------------------------------------------------------------------------

SEEDS = [bytes([0x30 + i]) * 32 for i in range(3)]
CRS = b"\xc5" * 32


@pytest.mark.parametrize("params,w", [((16, Q29, 7, 19), 4), ((16, Q60, 65537, 19), 16)])
def test_relinearization_identity_restated(params, w):
    sks, pk0, pk1, rlk0, rlk1 = ref_collective_keys(params, CRS, SEEDS, w)
    s = collective_secret(params, sks)
    assert np.array_equal(relin_residual(params, rlk0, rlk1, s, w), relin_noise(params, sks, SEEDS, w))
    # the collective public key is a key of s: pk0 + pk1 s = -sum_i e_i
    e = ref_aggregate(params, [error(ps, 6, 0, params[0], params[1], params[3]) for ps in SEEDS])
    assert np.array_equal(add(pk0, ring_mul(pk1, s, params[1]), q=params[1]), neg(e, params[1]))


def test_combine_is_decryption_under_the_collective_secret():
    params = (16, Q29, 7, 19)
    n, q, t = params[0], params[1], params[2]
    sks, pk0, pk1, _, _ = ref_collective_keys(params, CRS, SEEDS, 8)
    s = collective_secret(params, sks)
    rng = random.Random(5)
    # E = 0: exact for any pair of residues, not only for encryptions
    c0 = np.array([[rng.randrange(q) for _ in range(n)] for _ in range(2)], dtype=np.uint64)
    c1 = np.array([[rng.randrange(q) for _ in range(n)] for _ in range(2)], dtype=np.uint64)
    d = [ref_decrypt_share(params, sk, c1, bytes([9 + i]) * 32, 0, 0) for i, sk in enumerate(sks)]
    assert np.array_equal(ref_decrypt_combine(params, c0, d), ref_decrypt(params, s, c0, c1))
    # E > 0 on encryptions under the collective key: the plaintext comes back
    m = np.array([rng.randrange(-3, 4) % q for _ in range(n)], dtype=np.uint64)
    ct0, ct1 = ref_encrypt(params, pk0, pk1, m, b"\x44" * 32, 0)
    bound = (q // t // 2) // 3 // 8
    d = [ref_decrypt_share(params, sk, ct1, bytes([9 + i]) * 32, 7, bound) for i, sk in enumerate(sks)]
    assert np.array_equal(ref_decrypt_combine(params, ct0, d)[0], m)
    assert np.array_equal(ref_decrypt(params, s, ct0, ct1)[0], m)
    assert ref_noise(params, s, ct0, ct1, m) < (q // t) // 2


def test_one_party_is_the_single_key_scheme():
    params = (16, Q29, 7, 19)
    sk, pk0, pk1 = ref_keygen_share(params, SEEDS[0], SEEDS[0])
    assert set(int(x) for x in sk) <= {0, 1, params[1] - 1}
    c1 = uniform(b"\x01" * 32, 5, 3, 16, params[1])
    c0 = uniform(b"\x02" * 32, 5, 3, 16, params[1])
    d = ref_decrypt_share(params, sk, c1, b"\x03" * 32, 0, 0)
    assert np.array_equal(d[0], ring_mul(c1, sk, params[1]))
    assert np.array_equal(ref_decrypt_combine(params, c0, [d]), ref_decrypt(params, sk, c0, c1))


def test_smudging_sampler_range():
    q, bound = Q29, 3
    x = centred(smudge(b"\x05" * 32, (1 << 32) - 1, 4096, q, bound), q)
    assert min(x) == -bound and max(x) == bound
    assert list(smudge(b"\x05" * 32, 0, 64, q, 0)) == [0] * 64


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    for name in METHODS:
        assert callable(getattr(zk.Context, name)), name
    for word in ("domain 9", "domain 10", "11, 12, 13", "smudg", "party_seed", "NEVER REUSE"):
        assert word in header, word
    assert zk.PROF_BFV_SHARE_SUM == 12 and zk.PROF_BFV_DECRYPT_COMBINE == 13
    assert re.search(r"#define ZKFHE_PROF_BFV_SHARE_SUM 12\b", header) and re.search(r"#define ZKFHE_PROF_BFV_DECRYPT_COMBINE 13\b", header)
