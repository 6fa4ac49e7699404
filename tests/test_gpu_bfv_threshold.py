"""Threshold BFV on the GPU (bfv_threshold.hip): key shares, the two relinearization rounds, decryption shares and their combination
bit for bit against the restatements of tests/test_bfv_threshold_host.py, the smudging distribution, a relinearized product under the
collective key, the whole tally (proved encryptions, batch verification, sum, threshold decryption) and every refusal.
Run on the MI355X box: pytest -m gpu."""
import json
import os

import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60, relin_digits
from tests.test_bfv_threshold_host import (collective_secret, ref_aggregate, ref_decrypt, ref_decrypt_combine, ref_decrypt_share,
                                           ref_keygen_share, ref_noise, ref_relin_share1, ref_relin_share2, relin_noise,
                                           relin_residual, smudge)
from tests.test_gpu_bfv_encrypt import random_m
from tests.test_gpu_bfv_eval import plain_product

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K13 = (1024, Q29, 7, 19)   # the k = 13 parameters (examples/bfv.rs)
CRS = b"\xc5" * 32
PARTIES = [bytes([0x30 + i]) * 32 for i in range(16)]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def collective(ctx, params, seeds, w):
    """the key ceremony on the GPU: (sks, pk0, pk1, rlk0, rlk1, round-1 shares, round-2 shares)"""
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in seeds]
    sks = [k[0] for k in keys]
    pk0 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys]))
    r1 = [ctx.bfv_relin_share1(params, sk, CRS, ps, base_bits=w) for sk, ps in zip(sks, seeds)]
    hh = ctx.bfv_share_aggregate(params, np.array([np.concatenate(x) for x in r1]))   # h0 | h1: 2 l rows
    l = relin_digits(params[1], w)
    h0, h1 = hh[:l], hh[l:]
    r2 = [ctx.bfv_relin_share2(params, sk, ps, h0, h1, base_bits=w) for sk, ps in zip(sks, seeds)]
    rlk0 = ctx.bfv_share_aggregate(params, np.array(r2))
    return dict(sks=sks, keys=keys, pk0=pk0, pk1=keys[0][2], rlk0=rlk0, rlk1=h1, r1=r1, r2=r2, h0=h0)


def threshold_decrypt(ctx, params, sks, c0, c1, bound, tag):
    shares = [ctx.bfv_decrypt_share(params, sk, c1, seed=bytes([tag, i]) * 16, smudge_bound=bound) for i, sk in enumerate(sks)]
    return ctx.bfv_decrypt_combine(params, c0, np.array(shares))


# ---- 1. key shares ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [K13, (4096, Q60, 65537, 19), (16384, Q60, 65537, 19)])
def test_keygen_share_with_crs_equal_to_party_seed_is_fhe_keypair(ctx, params):
    seed = bytes(range(32))
    got, want = ctx.bfv_keygen_share(params, seed, seed), ctx.bfv_fhe_keypair(params, seed)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("params", [K13, (4096, Q60, 65537, 19)])
def test_key_shares_and_collective_pk_restated(ctx, params):
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES[:3]]
    for k, ps in zip(keys, PARTIES[:3]):
        for g, w in zip(k, ref_keygen_share(params, CRS, ps)):
            assert np.array_equal(g, w)
    assert all(np.array_equal(k[2], keys[0][2]) for k in keys)   # one CRS a
    pk0 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys]))
    assert pk0.shape == (params[0],) and np.array_equal(pk0, ref_aggregate(params, [k[1] for k in keys]))


# ---- 2. decryption shares --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [K13, (4096, Q60, 65537, 19)])
def test_decrypt_shares_restated(ctx, params):
    n, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(n)
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    c1 = rng.integers(0, q, size=(3, n), dtype=np.uint64)
    top = (q // t // 2) // 3 - 1   # floor(floor(Q/T)/2 / P) - 1 at P = 3
    for bound in (0, top, (q // t - 1) // 2):
        d = ctx.bfv_decrypt_share(params, sk, c1, seed=b"\x21" * 32, first_index=5, smudge_bound=bound)
        assert np.array_equal(d, ref_decrypt_share(params, sk, c1, b"\x21" * 32, 5, bound)), bound


def test_decrypt_shares_across_a_chunk(ctx):
    params = (16384, Q60, 65537, 19)
    n, q = params[0], params[1]
    rng = np.random.default_rng(129)
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[1])[0]
    c1 = rng.integers(0, q, size=(129, n), dtype=np.uint64)   # 128 ciphertexts per chunk at N = 16384
    d = ctx.bfv_decrypt_share(params, sk, c1, seed=b"\x22" * 32, first_index=3, smudge_bound=1000)
    for j in (0, 127, 128):
        assert np.array_equal(d[j], ref_decrypt_share(params, sk, c1[j], b"\x22" * 32, 3 + j, 1000)[0]), j
    one = ctx.bfv_decrypt_share(params, sk, c1[100:129], seed=b"\x22" * 32, first_index=103, smudge_bound=1000)
    assert np.array_equal(one, d[100:129])
    c0 = rng.integers(0, q, size=(129, n), dtype=np.uint64)
    d2 = ctx.bfv_decrypt_share(params, ctx.bfv_keygen_share(params, CRS, PARTIES[2])[0], c1, seed=b"\x23" * 32, smudge_bound=7)
    m = ctx.bfv_decrypt_combine(params, c0, np.array([d, d2]))
    for j in (0, 127, 128):
        assert np.array_equal(m[j], ref_decrypt_combine(params, c0[j], np.array([d[j], d2[j]]))[0]), j


def test_decrypt_share_index_spills_into_the_high_word(ctx):
    params = K13
    n, q = params[0], params[1]
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    c1 = np.random.default_rng(32).integers(0, q, size=(4, n), dtype=np.uint64)
    first = (1 << 32) - 2
    d = ctx.bfv_decrypt_share(params, sk, c1, seed=b"\x24" * 32, first_index=first, smudge_bound=50)
    assert np.array_equal(d, ref_decrypt_share(params, sk, c1, b"\x24" * 32, first, 50))


def test_smudging_distribution_chi_square(ctx):
    params = (16384, Q60, 65537, 19)
    n, q, bound = params[0], params[1], 3
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    d = ctx.bfv_decrypt_share(params, sk, np.zeros((64, n), dtype=np.uint64), seed=b"\x25" * 32, smudge_bound=bound)   # c1 = 0: d = e
    x = d.astype(np.int64).reshape(-1)   # residues below 2^60
    x = np.where(x > q // 2, x - q, x)
    assert x.size >= 10 ** 6 and x.min() == -bound and x.max() == bound
    counts = np.array([(x == v).sum() for v in range(-bound, bound + 1)], dtype=np.float64)
    exp = x.size / (2 * bound + 1)
    chi2 = ((counts - exp) ** 2 / exp).sum()
    assert chi2 < 6 + 8 * np.sqrt(12), (chi2, counts)
    assert np.array_equal(d[0][:8], smudge(b"\x25" * 32, 0, n, q, bound)[:8])


# ---- 4. combine ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [K13, (4096, Q60, 65537, 19)])
def test_one_party_combine_is_decrypt(ctx, params):
    n, q, t = params[0], params[1], params[2]
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x26" * 32)
    rng = np.random.default_rng(4)
    m = random_m(rng, (5, n), q, t)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x27" * 32)
    c0 = np.concatenate([ct["c0"], rng.integers(0, q, size=(3, n), dtype=np.uint64)])   # and arbitrary residues
    c1 = np.concatenate([ct["c1"], rng.integers(0, q, size=(3, n), dtype=np.uint64)])
    d = ctx.bfv_decrypt_share(params, sk, c1, seed=b"\x28" * 32, smudge_bound=0)
    got = ctx.bfv_decrypt_combine(params, c0, d[None])
    assert np.array_equal(got, ctx.bfv_decrypt(params, sk, c0, c1))
    assert np.array_equal(got[:5], m)


@pytest.mark.parametrize("n_parties", [3, 16])
def test_combine_restated(ctx, n_parties):
    params = K13
    n, q = params[0], params[1]
    rng = np.random.default_rng(n_parties)
    c0 = rng.integers(0, q, size=(6, n), dtype=np.uint64)
    d = rng.integers(0, q, size=(n_parties, 6, n), dtype=np.uint64)
    assert np.array_equal(ctx.bfv_decrypt_combine(params, c0, d), ref_decrypt_combine(params, c0, d))
    assert np.array_equal(ctx.bfv_share_aggregate(params, d), ref_aggregate(params, d))


# ---- 5. relinearization key ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", [(K13, 4), (K13, 8), ((4096, Q60, 65537, 19), 16)])
def test_relin_key_rounds_restated(ctx, params, w):
    seeds = PARTIES[:3]
    k = collective(ctx, params, seeds, w)
    for sk, ps, (h0_i, h1_i), r_i in zip(k["sks"], seeds, k["r1"], k["r2"]):
        w0, w1 = ref_relin_share1(params, sk, CRS, ps, w)
        assert np.array_equal(h0_i, w0) and np.array_equal(h1_i, w1)
        assert np.array_equal(r_i, ref_relin_share2(params, sk, ps, k["h0"], k["rlk1"], w))
    assert np.array_equal(k["h0"], ref_aggregate(params, [x[0] for x in k["r1"]]))
    assert np.array_equal(k["rlk1"], ref_aggregate(params, [x[1] for x in k["r1"]]))
    assert np.array_equal(k["rlk0"], ref_aggregate(params, k["r2"]))
    s = collective_secret(params, k["sks"])
    assert np.array_equal(relin_residual(params, k["rlk0"], k["rlk1"], s, w), relin_noise(params, k["sks"], seeds, w))


# ---- 6. a product under the collective key ---------------------------------------------------------------------------------

def test_product_under_the_collective_key(ctx):
    params, w = K13, 4
    n, q, t = params[:3]
    k = collective(ctx, params, PARTIES[:3], w)
    rng = np.random.default_rng(6)
    m = random_m(rng, (2, n), q, t)
    ct = ctx.bfv_encrypt(params, k["pk0"], k["pk1"], m, b"\x29" * 32)
    c0, c1 = ctx.bfv_mul(params, ct["c0"][:1], ct["c1"][:1], ct["c0"][1:], ct["c1"][1:], k["rlk0"], k["rlk1"], base_bits=w)
    want = plain_product(m[0], m[1], params)
    s = collective_secret(params, k["sks"])
    noise = ref_noise(params, s, c0, c1, want)
    assert noise < (q // t) // 2, noise
    assert np.array_equal(ref_decrypt(params, s, c0, c1)[0], want)
    assert np.array_equal(threshold_decrypt(ctx, params, k["sks"], c0, c1, 1 << 10, 0x60)[0], want)


# ---- 7. the tally end to end -----------------------------------------------------------------------------------------------

def test_threshold_tally_end_to_end(ctx):
    import zk_fhe_amd as zk
    from oracle import circuit_ref as C
    from zk_fhe_amd import inputs
    prm = C.BfvParams()
    params = (1024, prm.Q, prm.T, prm.B)
    assert params == K13
    n, q, t = params[:3]
    k = collective(ctx, params, PARTIES[:3], 8)
    cfgj = json.load(open(os.path.join(HERE, "golden", "bfv", "bfv_config.json")))
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), params, zk.BfvConfig.from_pinning(cfgj), replay=True)
    try:
        m = random_m(np.random.default_rng(77), (16, n), q, t)
        c0, c1, proofs, insts = pk.encrypt_and_prove(k["pk0"], k["pk1"], m, enc_seed=b"\x2a" * 32, seed=b"tally")
        res = zk.bfv_verify_batch(ctx, pk.export_vk(), list(zip(insts, proofs)))
        assert all(ok for ok, _ in res), [why for ok, why in res if not ok]
    finally:
        pk.destroy()
        srs.destroy()
    s0, s1 = ctx.bfv_sum(params, c0, c1)
    bound = 1 << 20
    assert 3 * bound < (q // t) // 2 // 10
    got = threshold_decrypt(ctx, params, k["sks"], s0, s1, bound, 0x70)[0]
    total = m.astype(object)
    total = np.where(total > q // 2, total - q, total).sum(axis=0)
    want = np.array([((int(v) % t) - t if (int(v) % t) > t // 2 else int(v) % t) % q for v in total], dtype=np.uint64)
    assert np.array_equal(got, want)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import zk_fhe_amd as zk
    params = K13
    n, q, t = params[:3]
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    c = np.random.default_rng(8).integers(0, q, size=(2, n), dtype=np.uint64)
    big = c.copy()
    big[1, 7] = q
    bad_sk = sk.copy()
    bad_sk[3] = 2
    l = relin_digits(q, 8)
    h = np.zeros((l, n), dtype=np.uint64)
    hbig = h.copy()
    hbig[l - 1, 0] = q
    E = "bad argument"
    cases = [
        (lambda: ctx.bfv_share_aggregate(params, np.zeros((0, n), dtype=np.uint64)), E),
        (lambda: ctx.bfv_share_aggregate(params, big), "bfv_share_aggregate: a share coefficient is not below Q"),
        (lambda: ctx.bfv_relin_share1(params, bad_sk, CRS, PARTIES[0]), r"bfv_relin_share1: a secret-key coefficient is not in \{0, 1, Q - 1\}"),
        (lambda: ctx.bfv_relin_share1(params, sk, CRS, PARTIES[0], base_bits=0), r"bfv_relin_share1: base_bits must be in \[1, 32\]"),
        (lambda: ctx.bfv_relin_share1(params, sk, CRS, PARTIES[0], base_bits=33), r"bfv_relin_share1: base_bits must be in \[1, 32\]"),
        (lambda: ctx.bfv_relin_share2(params, bad_sk, PARTIES[0], h, h), r"bfv_relin_share2: a secret-key coefficient is not in \{0, 1, Q - 1\}"),
        (lambda: ctx.bfv_relin_share2(params, sk, PARTIES[0], hbig, h), "bfv_relin_share2: an h0 coefficient is not below Q"),
        (lambda: ctx.bfv_relin_share2(params, sk, PARTIES[0], h, hbig), "bfv_relin_share2: an h1 coefficient is not below Q"),
        (lambda: ctx.bfv_relin_share2(params, sk, PARTIES[0], h, h, base_bits=40), r"bfv_relin_share2: base_bits must be in \[1, 32\]"),
        (lambda: ctx.bfv_decrypt_share(params, bad_sk, c), r"bfv_decrypt_share: a secret-key coefficient is not in \{0, 1, Q - 1\}"),
        (lambda: ctx.bfv_decrypt_share(params, sk, big), "bfv_decrypt_share: a ciphertext coefficient is not below Q"),
        (lambda: ctx.bfv_decrypt_share(params, sk, c, smudge_bound=(q // t - 1) // 2 + 1),
         r"bfv_decrypt_share: 2 smudge_bound \+ 1 must not exceed floor\(Q/T\)"),
        (lambda: ctx.bfv_decrypt_share(params, sk, c, smudge_bound=(1 << 64) - 1), r"2 smudge_bound \+ 1 must not exceed"),
        (lambda: ctx.bfv_decrypt_share(params, sk, np.zeros((0, n), dtype=np.uint64)), E),
        (lambda: ctx.bfv_decrypt_combine(params, big, np.array([c])), "bfv_decrypt_combine: a ciphertext coefficient is not below Q"),
        (lambda: ctx.bfv_decrypt_combine(params, c, np.array([c, big])), "bfv_decrypt_combine: a decryption-share coefficient is not below Q"),
        (lambda: ctx.bfv_decrypt_combine(params, c, np.zeros((0, 2, n), dtype=np.uint64)), E),
        (lambda: ctx.bfv_keygen_share((1000, q, t, 19), CRS, PARTIES[0]), "bfv params"),
        (lambda: ctx.bfv_decrypt_combine((1024, q, q, 19), c, np.array([c])), "bfv params"),
    ]
    for call, msg in cases:
        with pytest.raises(zk.ZkfheError, match=msg):
            call()
    # the largest allowed bound is accepted; NULL arguments are refused by the C entry points themselves
    ctx.bfv_decrypt_share(params, sk, c, smudge_bound=(q // t - 1) // 2)
    import ctypes
    prm = zk.BfvParamsC(*params)
    untyped = ctypes.CDLL(zk.LIB_PATH)   # its own function objects: every argument may be None, counts included
    for fn in ("zkfhe_bfv_keygen_share", "zkfhe_bfv_share_aggregate", "zkfhe_bfv_relin_share1", "zkfhe_bfv_relin_share2",
               "zkfhe_bfv_decrypt_share", "zkfhe_bfv_decrypt_combine"):
        f = getattr(untyped, fn)
        nargs = {"zkfhe_bfv_keygen_share": 5, "zkfhe_bfv_share_aggregate": 4, "zkfhe_bfv_relin_share1": 6, "zkfhe_bfv_relin_share2": 6,
                 "zkfhe_bfv_decrypt_share": 7, "zkfhe_bfv_decrypt_combine": 5}[fn]
        assert f(ctx.h, ctypes.byref(prm), *([None] * nargs)) == -1, fn   # ZKFHE_EINVAL
        assert "bad argument" in ctx.lib.zkfhe_last_error(ctx.h).decode(), fn
