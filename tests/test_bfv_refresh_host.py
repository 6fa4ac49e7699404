"""Host side of collective refresh and public collective key switching (no GPU): pure-Python restatements of the four calls of
zkfhe.h "Collective refresh and key switching", built from the helpers of tests/test_bfv_threshold_host.py, and at N = 16 what the
protocols promise: a refreshed ciphertext decrypts to the same plaintext with noise at most P B + (P + 1) (Q mod T), whatever the
input's noise was; a switched one decrypts under the recipient's key, with exactly the noise -u e' + sum e0 + (sum e1) s'; a second
committee opens it with its own shares.  Also the declarations and exports.  tests/test_gpu_bfv_refresh.py imports the restatements."""
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60
from tests.test_bfv_threshold_host import (add, collective_secret, error, neg, ref_aggregate, ref_collective_keys, ref_decrypt,
                                           ref_decrypt_combine, ref_decrypt_share, ref_encrypt, ref_keygen_share, ref_noise, ring_mul,
                                           ternary, uniform, uniform_ints)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_pcks_share", "zkfhe_bfv_pcks_combine", "zkfhe_bfv_refresh_share", "zkfhe_bfv_refresh_combine"]
METHODS = ["bfv_pcks_share", "bfv_pcks_combine", "bfv_refresh_share", "bfv_refresh_combine"]
DOM_PCKS_U, DOM_PCKS_E0, DOM_PCKS_E1, DOM_RFR_A, DOM_RFR_M, DOM_RFR_E0, DOM_RFR_E1 = 16, 17, 18, 19, 20, 21, 22


# ---- the four calls, restated from zkfhe.h -------------------------------------------------------------------------------------

def smudging(seed, domain, index, n, q, bound):
    """uniform mod 2E + 1, minus E, as residues mod Q"""
    return np.array([(x - bound) % q for x in uniform_ints(seed, domain, index, n, 2 * bound + 1)], dtype=np.uint64)


def scaled_mask(seed, index, n, q, t):
    """delta M for the refresh mask M of (seed, 20, index): uniform mod T"""
    return np.array([(q // t) * x % q for x in uniform_ints(seed, DOM_RFR_M, index, n, t)], dtype=np.uint64)


def ref_pcks_share(params, s, pk0_to, pk1_to, c1, seed, first_index, bound):
    n, q, b = params[0], params[1], params[3]
    c1 = np.asarray(c1, dtype=np.uint64).reshape(-1, n)
    h0, h1 = [], []
    for j in range(c1.shape[0]):
        u = ternary(seed, DOM_PCKS_U, first_index + j, n, q)
        h0.append(add(ring_mul(c1[j], s, q), ring_mul(pk0_to, u, q), smudging(seed, DOM_PCKS_E0, first_index + j, n, q, bound), q=q))
        h1.append(add(ring_mul(pk1_to, u, q), error(seed, DOM_PCKS_E1, first_index + j, n, q, b), q=q))
    return np.array(h0), np.array(h1)


def plane_sum(x, q):
    return np.asarray(x, dtype=np.uint64).astype(object).sum(axis=0) % q


def ref_pcks_combine(params, c0, h0, h1):
    n, q = params[0], params[1]
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1, n)
    h0 = np.asarray(h0, dtype=np.uint64).reshape(-1, c0.shape[0], n)
    h1 = np.asarray(h1, dtype=np.uint64).reshape(-1, c0.shape[0], n)
    return ((c0.astype(object) + plane_sum(h0, q)) % q).astype(np.uint64), plane_sum(h1, q).astype(np.uint64)


def ref_refresh_share(params, s, crs_seed, c1, seed, first_index, bound):
    n, q, t, b = params
    c1 = np.asarray(c1, dtype=np.uint64).reshape(-1, n)
    h0, h1 = [], []
    for j in range(c1.shape[0]):
        a = uniform(crs_seed, DOM_RFR_A, first_index + j, n, q)
        dm = scaled_mask(seed, first_index + j, n, q, t)
        h0.append(add(ring_mul(c1[j], s, q), neg(dm, q), smudging(seed, DOM_RFR_E0, first_index + j, n, q, bound), q=q))
        h1.append(add(neg(ring_mul(a, s, q), q), dm, error(seed, DOM_RFR_E1, first_index + j, n, q, b), q=q))
    return np.array(h0), np.array(h1)


def ref_refresh_combine(params, crs_seed, c0, h0, h1, first_index):
    n, q, t = params[0], params[1], params[2]
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1, n)
    h0 = np.asarray(h0, dtype=np.uint64).reshape(-1, c0.shape[0], n)
    h1 = np.asarray(h1, dtype=np.uint64).reshape(-1, c0.shape[0], n)
    v, w = (c0.astype(object) + plane_sum(h0, q)) % q, plane_sum(h1, q)
    out0 = [[((q // t) * (((2 * t * int(x) + q) // (2 * q)) % t) + int(y)) % q for x, y in zip(rv, rw)] for rv, rw in zip(v, w)]
    out1 = [uniform(crs_seed, DOM_RFR_A, first_index + j, n, q) for j in range(c0.shape[0])]
    return np.array(out0, dtype=np.uint64), np.array(out1, dtype=np.uint64)


def refresh_noise_bound(params, n_parties):
    """P B + (P + 1) (Q mod T): the noise of a refreshed ciphertext (zkfhe.h)"""
    return n_parties * params[3] + (n_parties + 1) * (params[1] % params[2])


def ref_refresh(params, sks, crs_seed, c0, c1, seeds, first_index, bound):
    shares = [ref_refresh_share(params, sk, crs_seed, c1, sd, first_index, bound) for sk, sd in zip(sks, seeds)]
    return ref_refresh_combine(params, crs_seed, c0, [x[0] for x in shares], [x[1] for x in shares], first_index)


# ---- tests -------------------------------------------------------------------------------------------------------------------

SEEDS = [bytes([0x30 + i]) * 32 for i in range(3)]
SHARE_SEEDS = [bytes([0x50 + i]) * 32 for i in range(3)]
CRS, CRS_REFRESH, CRS_OTHER = b"\xc5" * 32, b"\xc6" * 32, b"\xc7" * 32
PARAMS = [(16, Q29, 7, 19), (16, Q60, 65537, 19)]
BOUND = 1 << 10


def random_plain(rng, n, q, t):
    return np.array([rng.randrange(-((t - 1) // 2), t // 2 + 1) % q for _ in range(n)], dtype=np.uint64)


@pytest.fixture(scope="module", params=PARAMS, ids=["Q29", "Q60"])
def committee(request):
    """one committee of three and one encryption under its collective key, shared by the tests below and left unchanged"""
    params = request.param
    n, q, t = params[:3]
    sks, pk0, pk1, _, _ = ref_collective_keys(params, CRS, SEEDS, 8)
    m = random_plain(random.Random(n + t), n, q, t)
    c0, c1 = ref_encrypt(params, pk0, pk1, m, b"\x44" * 32, 0)
    return dict(params=params, sks=sks, s=collective_secret(params, sks), m=m, c0=c0, c1=c1)


@pytest.mark.parametrize("worn", [False, True], ids=["fresh", "noise_delta_8"])
def test_refresh_restated(committee, worn):
    params, sks, s, m = (committee[k] for k in ("params", "sks", "s", "m"))
    n, q, t = params[:3]
    delta, first = q // t, 5
    c0, c1 = committee["c0"], committee["c1"]
    if worn:   # a known error of size delta / 8 on c0, both signs
        c0 = add(c0, np.array([(delta // 8) * (-1) ** i % q for i in range(n)], dtype=np.uint64), q=q)
        fresh = ref_noise(params, s, committee["c0"], c1, m)
        assert delta // 8 - fresh <= ref_noise(params, s, c0, c1, m) <= delta // 8 + fresh
    # the sufficient condition of zkfhe.h holds for this input
    assert ref_noise(params, s, c0, c1, m) + 3 * BOUND + 4 * (q % t) < delta // 2 - t
    o0, o1 = ref_refresh(params, sks, CRS_REFRESH, c0, c1, SHARE_SEEDS, first, BOUND)
    assert np.array_equal(ref_decrypt(params, s, o0, o1)[0], m)
    assert ref_noise(params, s, o0, o1, m) <= refresh_noise_bound(params, 3)
    assert np.array_equal(o1[0], uniform(CRS_REFRESH, DOM_RFR_A, first, n, q))   # out1 is the CRS stream of domain 19


def test_pcks_to_a_single_recipient(committee):
    params, sks, s, m, c0, c1 = (committee[k] for k in ("params", "sks", "s", "m", "c0", "c1"))
    n, q, b = params[0], params[1], params[3]
    first, seed_to = 9, b"\x61" * 32
    s_to, pk0_to, pk1_to = ref_keygen_share(params, seed_to, seed_to)
    e_to = error(seed_to, 6, 0, n, q, b)
    assert np.array_equal(add(pk0_to, ring_mul(pk1_to, s_to, q), q=q), neg(e_to, q))   # pk0' + pk1' s' = -e'
    shares = [ref_pcks_share(params, sk, pk0_to, pk1_to, c1, sd, first, BOUND) for sk, sd in zip(sks, SHARE_SEEDS)]
    o0, o1 = ref_pcks_combine(params, c0, [x[0] for x in shares], [x[1] for x in shares])
    assert np.array_equal(ref_decrypt(params, s_to, o0, o1)[0], m)
    # [out0 + out1 s'] - [c0 + c1 s] = -u e' + sum e0 + (sum e1) s', rebuilt from the seeds
    u = ref_aggregate(params, [ternary(sd, DOM_PCKS_U, first, n, q) for sd in SHARE_SEEDS])
    e0 = ref_aggregate(params, [smudging(sd, DOM_PCKS_E0, first, n, q, BOUND) for sd in SHARE_SEEDS])
    e1 = ref_aggregate(params, [error(sd, DOM_PCKS_E1, first, n, q, b) for sd in SHARE_SEEDS])
    got = add(o0[0], ring_mul(o1[0], s_to, q), neg(add(c0, ring_mul(c1, s, q), q=q), q), q=q)
    assert np.array_equal(got, add(neg(ring_mul(u, e_to, q), q), e0, ring_mul(e1, s_to, q), q=q))


def test_pcks_to_a_second_committee(committee):
    params, sks, m, c0, c1 = (committee[k] for k in ("params", "sks", "m", "c0", "c1"))
    keys = [ref_keygen_share(params, CRS_OTHER, bytes([0x70 + i]) * 32) for i in range(2)]
    pk0_to, pk1_to = ref_aggregate(params, [k[1] for k in keys]), keys[0][2]
    shares = [ref_pcks_share(params, sk, pk0_to, pk1_to, c1, sd, 0, BOUND) for sk, sd in zip(sks, SHARE_SEEDS)]
    o0, o1 = ref_pcks_combine(params, c0, [x[0] for x in shares], [x[1] for x in shares])
    d = [ref_decrypt_share(params, k[0], o1, bytes([0x78 + i]) * 32, 0, BOUND) for i, k in enumerate(keys)]
    assert np.array_equal(ref_decrypt_combine(params, o0, d)[0], m)


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    for name in METHODS:
        assert callable(getattr(zk.Context, name)), name
    assert zk.PROF_BFV_PCKS_COMBINE == 21 and zk.PROF_BFV_REFRESH_COMBINE == 22
    assert re.search(r"#define ZKFHE_PROF_BFV_PCKS_COMBINE 21\b", header) and re.search(r"#define ZKFHE_PROF_BFV_REFRESH_COMBINE 22\b", header)
    for d in range(16, 23):
        assert re.search(r"domain %d\b" % d, header), d
    for word in ("Collective refresh and key switching", "NEVER REUSE", "Correctness condition", "Noise bound", "CRS agreement"):
        assert word in header, word
