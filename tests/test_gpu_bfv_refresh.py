"""Collective refresh and public collective key switching on the GPU (bfv_refresh.hip): the four calls bit for bit against the
restatements of tests/test_bfv_refresh_host.py, the combines on arbitrary planes, every call across its chunk boundary, one party
against zkfhe_bfv_decrypt, a second product after a refresh at the k = 13 parameters, the hand-over of its result to a second
committee, and every refusal in its order.  Run on the MI355X box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60, Q63
from tests.test_bfv_refresh_host import (ref_pcks_combine, ref_pcks_share, ref_refresh_combine, ref_refresh_share,
                                         refresh_noise_bound)
from tests.test_bfv_threshold_host import collective_secret, ref_decrypt, ref_noise
from tests.test_gpu_bfv_encrypt import random_m
from tests.test_gpu_bfv_eval import plain_product
from tests.test_gpu_bfv_threshold import collective, threshold_decrypt

pytestmark = pytest.mark.gpu
K13 = (1024, Q29, 7, 19)   # the k = 13 parameters (examples/bfv.rs)
CRS, CRS_REFRESH, CRS_OTHER = b"\xc5" * 32, b"\xc6" * 32, b"\xc7" * 32
PARTIES = [bytes([0x30 + i]) * 32 for i in range(3)]
SHARE_SEEDS = [bytes([0x50 + i]) * 32 for i in range(3)]
FIRST = (1 << 32) - 2   # the index of the second ciphertext crosses into the high word


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def plane_chunk(n, planes):
    """ciphertexts per chunk of a call that keeps `planes` planes resident (the rule in the header of bfv_refresh.hip)"""
    return max(1, max(8, (1 << 21) // n) * 4 // planes)


def refresh(ctx, params, sks, crs, c0, c1, first, bound, tag):
    shares = [ctx.bfv_refresh_share(params, sk, crs, c1, seed=bytes([tag, i]) * 16, first_index=first, smudge_bound=bound)
              for i, sk in enumerate(sks)]
    return ctx.bfv_refresh_combine(params, crs, c0, np.array([x[0] for x in shares]), np.array([x[1] for x in shares]), first_index=first)


def pcks(ctx, params, sks, pk0_to, pk1_to, c0, c1, first, bound, tag):
    shares = [ctx.bfv_pcks_share(params, sk, pk0_to, pk1_to, c1, seed=bytes([tag, i]) * 16, first_index=first, smudge_bound=bound)
              for i, sk in enumerate(sks)]
    return ctx.bfv_pcks_combine(params, c0, np.array([x[0] for x in shares]), np.array([x[1] for x in shares]))


# ---- 1. bit for bit against the restatements ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bound", [0, 1000])
@pytest.mark.parametrize("params", [(8, Q63, 97, 19), K13, (4096, Q60, 65537, 19)], ids=["N8_Q63", "K13", "N4096_Q60"])
def test_all_four_calls_restated(ctx, params, bound):
    n, q = params[0], params[1]
    rng = np.random.default_rng(n + bound)
    sks = [ctx.bfv_keygen_share(params, CRS, ps)[0] for ps in PARTIES]
    _, pk0_to, pk1_to = ctx.bfv_fhe_keypair(params, b"\x61" * 32)
    c0 = rng.integers(0, q, size=(3, n), dtype=np.uint64)   # the calls are exact for any residues
    c1 = rng.integers(0, q, size=(3, n), dtype=np.uint64)
    rs, ks = [], []
    for sk, sd in zip(sks, SHARE_SEEDS):
        rs.append(ctx.bfv_refresh_share(params, sk, CRS_REFRESH, c1, seed=sd, first_index=FIRST, smudge_bound=bound))
        for g, w in zip(rs[-1], ref_refresh_share(params, sk, CRS_REFRESH, c1, sd, FIRST, bound)):
            assert g.shape == (3, n) and np.array_equal(g, w)
        ks.append(ctx.bfv_pcks_share(params, sk, pk0_to, pk1_to, c1, seed=sd, first_index=FIRST, smudge_bound=bound))
        for g, w in zip(ks[-1], ref_pcks_share(params, sk, pk0_to, pk1_to, c1, sd, FIRST, bound)):
            assert g.shape == (3, n) and np.array_equal(g, w)
    h0, h1 = np.array([x[0] for x in rs]), np.array([x[1] for x in rs])
    for g, w in zip(ctx.bfv_refresh_combine(params, CRS_REFRESH, c0, h0, h1, first_index=FIRST),
                    ref_refresh_combine(params, CRS_REFRESH, c0, h0, h1, FIRST)):
        assert g.shape == (3, n) and np.array_equal(g, w)
    h0, h1 = np.array([x[0] for x in ks]), np.array([x[1] for x in ks])
    for g, w in zip(ctx.bfv_pcks_combine(params, c0, h0, h1), ref_pcks_combine(params, c0, h0, h1)):
        assert g.shape == (3, n) and np.array_equal(g, w)


# ---- 2. the combines on arbitrary planes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_parties", [1, 16])
def test_combine_planes_restated(ctx, n_parties):
    params = K13
    n, q = params[0], params[1]
    rng = np.random.default_rng(100 + n_parties)
    c0 = rng.integers(0, q, size=(6, n), dtype=np.uint64)
    h0 = rng.integers(0, q, size=(n_parties, 6, n), dtype=np.uint64)
    h1 = rng.integers(0, q, size=(n_parties, 6, n), dtype=np.uint64)
    for g, w in zip(ctx.bfv_pcks_combine(params, c0, h0, h1), ref_pcks_combine(params, c0, h0, h1)):
        assert np.array_equal(g, w)
    for g, w in zip(ctx.bfv_refresh_combine(params, CRS_REFRESH, c0, h0, h1, first_index=7), ref_refresh_combine(params, CRS_REFRESH, c0, h0, h1, 7)):
        assert np.array_equal(g, w)


# ---- 3. across a chunk boundary, GPU against GPU -----------------------------------------------------------------------------

def in_two_parts(call, count, cut):
    """call(lo, hi, first_index) over [0, cut) and [cut, count), the second with the index advanced, joined per output"""
    a, b = call(0, cut, 3), call(cut, count, 3 + cut)
    return [np.concatenate([x, y]) for x, y in zip(a, b)]


def test_shares_across_a_chunk(ctx):
    params = K13
    n, q = params[0], params[1]
    rng = np.random.default_rng(820)
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    _, pk0_to, pk1_to = ctx.bfv_fhe_keypair(params, b"\x62" * 32)
    count = plane_chunk(n, 9) + 1   # one more than the larger of the two share chunks: 910 (PCKS) and 819 (refresh)
    assert plane_chunk(n, 10) + 1 == 820 and count == 911
    c1 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
    for cnt, call in (
            (plane_chunk(n, 10) + 1,
             lambda lo, hi, first: ctx.bfv_refresh_share(params, sk, CRS_REFRESH, c1[lo:hi], seed=b"\x63" * 32, first_index=first, smudge_bound=1000)),
            (count,
             lambda lo, hi, first: ctx.bfv_pcks_share(params, sk, pk0_to, pk1_to, c1[lo:hi], seed=b"\x64" * 32, first_index=first, smudge_bound=1000))):
        whole = call(0, cnt, 3)
        for g, w in zip(whole, in_two_parts(call, cnt, 300)):
            assert g.shape == (cnt, n) and np.array_equal(g, w)
        assert not np.array_equal(whole[0][cnt - 2], whole[0][cnt - 1])


def test_combines_across_a_chunk(ctx):
    params, n_parties = K13, 2
    n, q = params[0], params[1]
    count = plane_chunk(n, 2 * n_parties + 3) + 1
    assert count == 1171
    rng = np.random.default_rng(1171)
    c0 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
    h0 = rng.integers(0, q, size=(n_parties, count, n), dtype=np.uint64)
    h1 = rng.integers(0, q, size=(n_parties, count, n), dtype=np.uint64)
    for call in (lambda lo, hi, first: ctx.bfv_refresh_combine(params, CRS_REFRESH, c0[lo:hi], h0[:, lo:hi], h1[:, lo:hi], first_index=first),
                 lambda lo, hi, first: ctx.bfv_pcks_combine(params, c0[lo:hi], h0[:, lo:hi], h1[:, lo:hi])):
        for g, w in zip(call(0, count, 3), in_two_parts(call, count, 300)):
            assert g.shape == (count, n) and np.array_equal(g, w)
    # the last ciphertext, past the boundary, against the restatement
    got = ctx.bfv_refresh_combine(params, CRS_REFRESH, c0, h0, h1, first_index=3)
    want = ref_refresh_combine(params, CRS_REFRESH, c0[-1], h0[:, -1], h1[:, -1], 3 + count - 1)
    assert np.array_equal(got[0][-1], want[0][0]) and np.array_equal(got[1][-1], want[1][0])


# ---- 4. one party ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [K13, (4096, Q60, 65537, 19)], ids=["K13", "N4096_Q60"])
def test_one_party_refresh_then_decrypt(ctx, params):
    n, q, t = params[:3]
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x65" * 32)
    m = random_m(np.random.default_rng(5), (5, n), q, t)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x66" * 32)
    r0, r1 = refresh(ctx, params, [sk], CRS_REFRESH, ct["c0"], ct["c1"], 11, 0, 0x67)
    want = ctx.bfv_decrypt(params, sk, ct["c0"], ct["c1"])
    assert np.array_equal(ctx.bfv_decrypt(params, sk, r0, r1), want) and np.array_equal(want, m)
    assert int(ctx.bfv_noise(params, sk, r0, r1).max()) <= refresh_noise_bound(params, 1)


# ---- 5. depth beyond one, and 6. the hand-over -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deep(ctx):
    """at the k = 13 parameters with w = 4 and three parties: p = ct0 * ct1, r = refresh(p) with E = 2^10, p2 = r * ct2"""
    params, w = K13, 4
    n, q, t = params[:3]
    k = collective(ctx, params, PARTIES, w)
    m = random_m(np.random.default_rng(6), (3, n), q, t)
    ct = ctx.bfv_encrypt(params, k["pk0"], k["pk1"], m, b"\x29" * 32)
    mul = lambda a0, a1, j: ctx.bfv_mul(params, a0, a1, ct["c0"][j:j + 1], ct["c1"][j:j + 1], k["rlk0"], k["rlk1"], base_bits=w)  # noqa: E731
    p = mul(ct["c0"][:1], ct["c1"][:1], 1)
    r = refresh(ctx, params, k["sks"], CRS_REFRESH, p[0], p[1], 0, 1 << 10, 0x68)
    p2 = mul(r[0], r[1], 2)
    m01 = plain_product(m[0], m[1], params)
    return dict(params=params, sks=k["sks"], s=collective_secret(params, k["sks"]), p=p, r=r, p2=p2, m01=m01,
                m012=plain_product(m01, m[2], params))


def test_a_second_product_after_a_refresh(ctx, deep):
    params, s = deep["params"], deep["s"]
    q, t = params[1], params[2]
    noise_p, noise_r = ref_noise(params, s, *deep["p"], deep["m01"]), ref_noise(params, s, *deep["r"], deep["m01"])
    print("noise of the product %d, of the refreshed product %d, floor(Q/T)/2 = %d" % (noise_p, noise_r, q // t // 2))
    assert refresh_noise_bound(params, 3) == 61
    assert noise_r <= 61 < noise_p
    noise_p2 = ref_noise(params, s, *deep["p2"], deep["m012"])
    print("noise of the second product %d" % noise_p2)
    assert noise_p2 < (q // t) // 2
    assert np.array_equal(ref_decrypt(params, s, *deep["p2"])[0], deep["m012"])
    assert np.array_equal(threshold_decrypt(ctx, params, deep["sks"], *deep["p2"], 1 << 10, 0x69)[0], deep["m012"])


def test_hand_over_to_a_second_committee(ctx, deep):
    params = deep["params"]
    keys = [ctx.bfv_keygen_share(params, CRS_OTHER, bytes([0x70 + i]) * 32) for i in range(2)]
    pk0_to = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys]))
    o0, o1 = pcks(ctx, params, deep["sks"], pk0_to, keys[0][2], *deep["p2"], 0, 1 << 10, 0x6a)
    got = threshold_decrypt(ctx, params, [k[0] for k in keys], o0, o1, 1 << 10, 0x6b)
    assert np.array_equal(got[0], deep["m012"])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------


def test_refusals_in_order_and_outputs_untouched(ctx):
    import zk_fhe_amd as zk
    params = K13
    n, q, t = params[:3]
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    _, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x6c" * 32)
    c = np.random.default_rng(8).integers(0, q, size=(2, n), dtype=np.uint64)
    hs = np.array([c, c])   # two parties
    big, bad_sk, big_pk = c.copy(), sk.copy(), pk1.copy()
    big[1, 7], bad_sk[3], big_pk[n - 1] = q, 2, q
    hbig = np.array([c, big])
    too_wide, seed, bad_params = (q // t - 1) // 2 + 1, b"\x6d" * 32, (1000, q, t, 19)
    PS, PC, RS, RC = "zkfhe_bfv_pcks_share", "zkfhe_bfv_pcks_combine", "zkfhe_bfv_refresh_share", "zkfhe_bfv_refresh_combine"
    ps = lambda prm=params, sk=sk, pk0=pk0, pk1=pk1, n_cts=2, c1=c, e=0: (PS, prm, (sk, pk0, pk1, n_cts, c1, seed, 0, e))  # noqa: E731
    rs = lambda prm=params, sk=sk, n_cts=2, c1=c, e=0: (RS, prm, (sk, CRS_REFRESH, n_cts, c1, seed, 0, e))  # noqa: E731
    pc = lambda prm=params, p=2, n_cts=2, c0=c, h0=hs, h1=hs: (PC, prm, (p, n_cts, c0, h0, h1))  # noqa: E731
    rc = lambda prm=params, p=2, n_cts=2, c0=c, h0=hs, h1=hs: (RC, prm, (p, n_cts, CRS_REFRESH, 0, c0, h0, h1))  # noqa: E731
    zero, wide, ternary_msg = "a NULL argument or a zero count", r"2 smudge_bound \+ 1 must not exceed floor\(Q/T\)", \
        r"a secret-key coefficient is not in \{0, 1, Q - 1\}"
    cases = [
        # 1. a zero count or bad parameters, before everything else
        (ps(n_cts=0, e=too_wide, c1=big, sk=bad_sk), "bfv_pcks_share: " + zero),
        (rs(n_cts=0, e=too_wide, c1=big, sk=bad_sk), "bfv_refresh_share: " + zero),
        (pc(p=0, c0=big), "bfv_pcks_combine: " + zero), (pc(n_cts=0, c0=big), "bfv_pcks_combine: " + zero),
        (rc(p=0, c0=big), "bfv_refresh_combine: " + zero), (rc(n_cts=0, c0=big), "bfv_refresh_combine: " + zero),
        (ps(prm=bad_params, e=too_wide, c1=big), "bfv params"), (rs(prm=bad_params, e=too_wide, c1=big), "bfv params"),
        (pc(prm=bad_params, c0=big), "bfv params"), (rc(prm=(1024, q, q, 19), c0=big), "bfv params"),
        # 2. the smudging bound, before the range of the inputs
        (ps(e=too_wide, c1=big, sk=bad_sk), "bfv_pcks_share: " + wide), (ps(e=(1 << 64) - 1), "bfv_pcks_share: " + wide),
        (rs(e=too_wide, c1=big, sk=bad_sk), "bfv_refresh_share: " + wide), (rs(e=(1 << 64) - 1), "bfv_refresh_share: " + wide),
        # 3. a coefficient >= Q, before the secret key
        (ps(c1=big, sk=bad_sk), "bfv_pcks_share: a ciphertext coefficient is not below Q"),
        (ps(pk0=big_pk, sk=bad_sk), "bfv_pcks_share: a public-key coefficient is not below Q"),
        (ps(pk1=big_pk, sk=bad_sk), "bfv_pcks_share: a public-key coefficient is not below Q"),
        (rs(c1=big, sk=bad_sk), "bfv_refresh_share: a ciphertext coefficient is not below Q"),
        (pc(c0=big), "bfv_pcks_combine: a ciphertext coefficient is not below Q"),
        (pc(h0=hbig), "bfv_pcks_combine: a share coefficient is not below Q"), (pc(h1=hbig), "bfv_pcks_combine: a share coefficient is not below Q"),
        (rc(c0=big), "bfv_refresh_combine: a ciphertext coefficient is not below Q"),
        (rc(h0=hbig), "bfv_refresh_combine: a share coefficient is not below Q"), (rc(h1=hbig), "bfv_refresh_combine: a share coefficient is not below Q"),
        # 4. a non-ternary secret key
        (ps(sk=bad_sk), "bfv_pcks_share: " + ternary_msg), (rs(sk=bad_sk), "bfv_refresh_share: " + ternary_msg),
    ]
    mark = np.uint64(0xA5A5A5A5A5A5A5A5)
    for (fn, prm, args), msg in cases:
        outs = [np.full((2, n), mark, dtype=np.uint64) for _ in range(2)]
        with pytest.raises(zk.ZkfheError, match=msg):
            ctx._call(fn, prm, *args, *outs)
        assert all((o == mark).all() for o in outs), (fn, msg)
    # the largest allowed bound is accepted; NULL arguments are refused by the C entry points themselves
    ctx.bfv_pcks_share(params, sk, pk0, pk1, c, smudge_bound=too_wide - 1)
    ctx.bfv_refresh_share(params, sk, CRS_REFRESH, c, smudge_bound=too_wide - 1)
    prm = zk.BfvParamsC(*params)
    untyped = ctypes.CDLL(zk.LIB_PATH)   # its own function objects: every argument may be None, counts included
    for fn in (PS, PC, RS, RC):
        f = getattr(untyped, fn)
        assert f(ctx.h, ctypes.byref(prm), *([None] * (len(zk.SIGNATURES[fn][1]) - 2))) == -1, fn   # ZKFHE_EINVAL
        assert (fn[len("zkfhe_"):] + ": a NULL argument") in ctx.lib.zkfhe_last_error(ctx.h).decode(), fn
