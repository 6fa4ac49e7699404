"""Edges of the GPU BFV rotations, linear transforms and threshold calls (bfv_galois.hip, bfv_linear.hip, bfv_threshold.hip) that
their own test files do not reach: rings down to N = 8 with every odd g, ciphertext counts and giant-step counts across every tile
of the kernels, 600 elements, every digit width with even, power-of-two and tiny Q, T = 2 and T near Q, B = 1023, smudging bounds
at their ends, and the range rule at 150 / 151 bits with magnitudes near 2^146.  Every expectation is restated on Python integers
from the definitions in zkfhe.h, with the oracles of the host test files and the generators of
tests/test_bfv_rotation_edges_host.py.  Run on the MI355X box: pytest -m gpu."""
import functools

import numpy as np
import pytest

from tests.test_bfv_bsgs_host import bsgs_slots, ref_linear_transform_bsgs
from tests.test_bfv_edges_host import Q62, QE
from tests.test_bfv_eval_host import Q29, Q60, Q63, centred, relin_digits
from tests.test_bfv_galois_host import (encode, eval_slots, galois_element, plain_slot_sum, ref_apply_galois, ref_galois_key, rotate,
                                        sigma, slot_sum_elements)
from tests.test_bfv_linear_host import ref_hoisted_rotation, ref_linear_transform, transform_slots
from tests.test_bfv_rotation_edges_host import (EDGE, MANY, RINGS, SWEEP, WORST, in_ranges, many_elements, negated, nonzero_plaintexts,
                                                plaintexts, random_keys, range_bits, recomposition_key, residues, ring_elements,
                                                ring_steps, ring_width, sigma_sum, split, sweep_lists, width_rows, worst_case)
from tests.test_bfv_threshold_host import (add, collective_secret, neg, ref_aggregate, ref_decrypt_combine, ref_decrypt_share,
                                           ref_keygen_share, ref_relin_share1, ref_relin_share2, relin_noise, relin_residual, ring_mul,
                                           ternary, uniform)

pytestmark = pytest.mark.gpu
CRS = b"\xc8" * 32
PARTIES = [bytes([0x68 + i]) * 32 for i in range(3)]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


# ---- helpers -----------------------------------------------------------------------------------------------------------------

def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def keys_for(ctx, params, sk, elements, w, seed):
    """one key per distinct element, laid out per list entry (repeats share their rows)"""
    made = {g: ctx.bfv_galois_keygen(params, sk, g, seed=seed, base_bits=w) for g in set(elements)}
    return np.array([made[g][0] for g in elements]), np.array([made[g][1] for g in elements])


def errors(q, *terms):
    """the sum of `terms` mod Q read centred: the error sample left when everything else of a formula is subtracted"""
    return centred(add(*terms, q=q), q)


def gadget(s, j, w, q):
    """2^(j w) s mod Q for a ternary s"""
    return np.array([int(x) * (1 << (j * w)) % q for x in s], dtype=np.uint64)


def restate_four_calls(ctx, params, w, c0, c1, elements, gk0, gk1, diag, n_baby, bdiag, rows=None):
    """apply_galois per element, apply_galois_many, linear_transform and linear_transform_bsgs (the element list split as baby x
    giant after n_baby entries, bdiag of shape (n_giant, n_baby, N)) against their restatements, on the ciphertexts `rows`"""
    rows = range(c0.shape[0]) if rows is None else rows
    for k, g in enumerate(elements):
        o0, o1 = ctx.bfv_apply_galois(params, c0, c1, g, gk0[k], gk1[k], base_bits=w)
        for j in rows:
            assert same((o0[j], o1[j]), ref_apply_galois(params, c0[j], c1[j], g, gk0[k], gk1[k], w)), (g, j)
    m0, m1 = ctx.bfv_apply_galois_many(params, c0, c1, elements, gk0, gk1, base_bits=w)
    assert m0.shape == m1.shape == (len(elements),) + c0.shape
    for k, g in enumerate(elements):
        for j in rows:
            assert same((m0[k, j], m1[k, j]), ref_hoisted_rotation(params, c0[j], c1[j], g, gk0[k], gk1[k], w)), (g, j)
    t0, t1 = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    for j in rows:
        assert same((t0[j], t1[j]), ref_linear_transform(params, c0[j], c1[j], elements, gk0, gk1, w, diag)), j
    (gb, gg), nb = split(elements, n_baby), n_baby
    b0, b1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, gb, gk0[:nb], gk1[:nb], gg, gk0[nb:], gk1[nb:], bdiag, base_bits=w)
    for j in rows:
        want = ref_linear_transform_bsgs(params, c0[j], c1[j], gb, gk0[:nb], gk1[:nb], gg, gk0[nb:], gk1[nb:], w, bdiag)
        assert same((b0[j], b1[j]), want), j
    return (m0, m1), (t0, t1), (b0, b1)


# ---- 1. small rings, every call --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,t", RINGS)
def test_small_rings_every_call(ctx, n, t):
    import zk_fhe_amd as zk
    params, w = (n, Q60, t, 19), ring_width(n)
    q = params[1]
    rng = np.random.default_rng(n)
    steps, elements = ring_steps(n), ring_elements(n)
    assert zk.bfv_slot_count(params) == n and [zk.bfv_galois_element(params, k, sw) for k, sw in steps] == elements
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, bytes([n % 251]) * 32)
    # slots: encode and decode against interpolation and evaluation, the values 0 and T - 1 among them
    v = rng.integers(0, t, size=(3, n), dtype=np.uint64)
    v[0, 0], v[0, 1] = 0, t - 1
    v[2, :n // 2], v[2, n // 2:] = 0, t - 1
    m = ctx.bfv_encode_slots(params, v)
    for j in range(3):
        assert np.array_equal(m[j], encode(params, v[j])), j
    assert np.array_equal(ctx.bfv_decode_slots(params, m), v)
    p = plaintexts(rng, params, (1,))
    assert np.array_equal(ctx.bfv_decode_slots(params, p)[0], eval_slots(params, p[0]))
    # keys, g = 1 included
    seed = bytes([n % 251 + 1]) * 32
    gk0, gk1 = keys_for(ctx, params, sk, elements, w, seed)
    for k, g in enumerate(elements):
        assert same((gk0[k], gk1[k]), ref_galois_key(params, sk, seed, seed, g, w)), g
    # the four calls on two encryptions, bit for bit, and what they decrypt to
    ct = ctx.bfv_encrypt(params, pk0, pk1, m[:2], bytes([n % 251 + 2]) * 32)
    c0, c1 = ct["c0"], ct["c1"]
    nb = 3 if n == 8 else 2
    d = rng.integers(0, t, size=(len(elements), n), dtype=np.uint64)
    bd = rng.integers(0, t, size=(len(elements) - nb, nb, n), dtype=np.uint64)
    diag = ctx.bfv_encode_slots(params, d)
    bdiag = ctx.bfv_encode_slots(params, bd.reshape(-1, n)).reshape(bd.shape)
    rows = None if n <= 64 else [1]   # the restatements take a second per ciphertext at N = 2048; both decrypt below
    many, flat, bsgs = restate_four_calls(ctx, params, w, c0, c1, elements, gk0, gk1, diag, nb, bdiag, rows)
    limit = (q // t) // 2
    for j in range(2):
        for k in range(len(elements)):
            got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, many[0][k, j], many[1][k, j]))[0]
            assert np.array_equal(got, rotate(v[j], *steps[k])), (j, k)
        got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, flat[0][j], flat[1][j]))[0]
        assert np.array_equal(got, transform_slots(params, v[j], steps, d)), j
        got = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, bsgs[0][j], bsgs[1][j]))[0]
        assert np.array_equal(got, bsgs_slots(params, v[j], *split(steps, nb), bd)), j
    for x0, x1 in (flat, bsgs):
        assert int(ctx.bfv_noise(params, sk, x0, x1).max()) < limit
    # slot_sum: the composition x <- x + apply_galois(x, g) restated, and the plaintext it decrypts to
    sum_g = zk.bfv_slot_sum_elements(params)
    assert sum_g == slot_sum_elements(n)
    sk0, sk1 = keys_for(ctx, params, sk, sum_g, w, seed)
    s0, s1 = ctx.bfv_slot_sum(params, c0, c1, sk0, sk1, base_bits=w)
    x0, x1 = c0[0], c1[0]
    for k, g in enumerate(sum_g):
        r0, r1 = ref_apply_galois(params, x0, x1, g, sk0[k], sk1[k], w)
        x0, x1 = add(x0, r0, q=q), add(x1, r1, q=q)
    assert np.array_equal(s0[0], x0) and np.array_equal(s1[0], x1)
    dec = ctx.bfv_decrypt(params, sk, s0, s1)
    for j in range(2):
        assert np.array_equal(dec[j], plain_slot_sum(params, m[j])), j
        total = int(v[j].astype(object).sum()) % t
        assert np.array_equal(ctx.bfv_decode_slots(params, dec[j])[0], np.full(n, total, dtype=np.uint64)), j


@pytest.mark.parametrize("w", [1, 16])
@pytest.mark.parametrize("n,t", [RINGS[0], RINGS[2]])
def test_small_rings_threshold_calls(ctx, n, t, w):
    params = (n, Q60, t, 19)
    q = params[1]
    rng = np.random.default_rng(n + w)
    l = relin_digits(q, w)
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES]
    for k, ps in zip(keys, PARTIES):
        assert same(k, ref_keygen_share(params, CRS, ps))
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]
    assert np.array_equal(pk0, ref_aggregate(params, [k[1] for k in keys]))
    # the two relinearization rounds
    r1 = [ctx.bfv_relin_share1(params, sk, CRS, ps, base_bits=w) for sk, ps in zip(sks, PARTIES)]
    for sk, ps, got in zip(sks, PARTIES, r1):
        assert got[0].shape == (l, n) and same(got, ref_relin_share1(params, sk, CRS, ps, w))
    hh = ctx.bfv_share_aggregate(params, np.array([np.concatenate(x) for x in r1]))
    assert np.array_equal(hh, ref_aggregate(params, [np.concatenate(x) for x in r1]))
    h0, h1 = hh[:l], hh[l:]
    r2 = [ctx.bfv_relin_share2(params, sk, ps, h0, h1, base_bits=w) for sk, ps in zip(sks, PARTIES)]
    for sk, ps, got in zip(sks, PARTIES, r2):
        assert np.array_equal(got, ref_relin_share2(params, sk, ps, h0, h1, w))
    rlk0 = ctx.bfv_share_aggregate(params, np.array(r2))
    assert np.array_equal(rlk0, ref_aggregate(params, r2))
    assert np.array_equal(relin_residual(params, rlk0, h1, collective_secret(params, sks), w), relin_noise(params, sks, PARTIES, w))
    # collective Galois keys, a rotation under them and its threshold decryption
    v = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    m = ctx.bfv_encode_slots(params, v)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x6c" * 32)
    bound = 1 << 20
    for steps, swap in ((1, False), (0, True)):
        g = galois_element(n, steps, swap)
        shares = [ctx.bfv_galois_share(params, sk, CRS, ps, g, base_bits=w) for sk, ps in zip(sks, PARTIES)]
        for sk, ps, got in zip(sks, PARTIES, shares):
            assert same(got, ref_galois_key(params, sk, CRS, ps, g, w)), g
        gk0, gk1 = ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])), shares[0][1]
        assert np.array_equal(gk0, ref_aggregate(params, [s[0] for s in shares]))
        o0, o1 = ctx.bfv_apply_galois(params, ct["c0"], ct["c1"], g, gk0, gk1, base_bits=w)
        for j in range(2):
            assert same((o0[j], o1[j]), ref_apply_galois(params, ct["c0"][j], ct["c1"][j], g, gk0, gk1, w)), (g, j)
        d = [ctx.bfv_decrypt_share(params, sk, o1, seed=bytes([0x7a, i]) * 16, first_index=3, smudge_bound=bound) for i, sk in enumerate(sks)]
        for i, sk in enumerate(sks):
            assert np.array_equal(d[i], ref_decrypt_share(params, sk, o1, bytes([0x7a, i]) * 16, 3, bound)), (g, i)
        got = ctx.bfv_decrypt_combine(params, o0, np.array(d))
        assert np.array_equal(got, ref_decrypt_combine(params, o0, d))
        for j in range(2):
            assert np.array_equal(got[j], sigma(m[j], g, q)), (g, j)
            assert np.array_equal(ctx.bfv_decode_slots(params, got[j])[0], rotate(v[j], steps, swap)), (g, j)


# ---- 2. tile edges, swept at N = 16 -------------------------------------------------------------------------------------------------

SWEEP_W = 16
SWEEP_FLAT = [galois_element(16, 1), 1, 31, galois_element(16, 1), galois_element(16, 6, True)]


@functools.lru_cache(maxsize=None)
def sweep_inputs():
    """nine ciphertexts, random keys per list entry (repeats too) and full-range diagonals, shared by the sweeps"""
    rng = np.random.default_rng(16)
    x = dict(c0=residues(rng, SWEEP, 9), c1=residues(rng, SWEEP, 9), flat=random_keys(rng, SWEEP, 5, SWEEP_W),
             baby=random_keys(rng, SWEEP, 3, SWEEP_W), giant=random_keys(rng, SWEEP, 9, SWEEP_W),
             diag=plaintexts(rng, SWEEP, (5,)), grid=nonzero_plaintexts(rng, SWEEP, (9, 3)))
    for a in x.values():
        for b in (a if isinstance(a, tuple) else (a,)):
            b.setflags(write=False)
    assert in_ranges(SWEEP, cts=[x["c0"], x["c1"]], keys=x["flat"] + x["baby"] + x["giant"], diags=[x["diag"], x["grid"]], elements=SWEEP_FLAT)
    return x


@functools.lru_cache(maxsize=None)
def sweep_flat_ref(j):
    x = sweep_inputs()
    rot = [ref_hoisted_rotation(SWEEP, x["c0"][j], x["c1"][j], g, x["flat"][0][k], x["flat"][1][k], SWEEP_W) for k, g in enumerate(SWEEP_FLAT)]
    return rot, ref_linear_transform(SWEEP, x["c0"][j], x["c1"][j], SWEEP_FLAT, x["flat"][0], x["flat"][1], SWEEP_W, x["diag"])


@functools.lru_cache(maxsize=None)
def sweep_bsgs_ref(n_baby, n_giant, j):
    x = sweep_inputs()
    gb, gg = sweep_lists(n_baby, n_giant)
    return ref_linear_transform_bsgs(SWEEP, x["c0"][j], x["c1"][j], gb, x["baby"][0][:n_baby], x["baby"][1][:n_baby], gg,
                                     x["giant"][0][:n_giant], x["giant"][1][:n_giant], SWEEP_W, x["grid"][:n_giant, :n_baby])


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 9])
def test_ciphertext_tiles_of_the_flat_calls(ctx, c):
    x = sweep_inputs()
    c0, c1 = x["c0"][:c], x["c1"][:c]
    m0, m1 = ctx.bfv_apply_galois_many(SWEEP, c0, c1, SWEEP_FLAT, *x["flat"], base_bits=SWEEP_W)
    t0, t1 = ctx.bfv_linear_transform(SWEEP, c0, c1, SWEEP_FLAT, *x["flat"], x["diag"], base_bits=SWEEP_W)
    assert m0.shape == (5, c, 16) and t0.shape == (c, 16)
    for j in range(c):
        rot, lin = sweep_flat_ref(j)
        for k in range(5):
            assert same((m0[k, j], m1[k, j]), rot[k]), (j, k)
        assert same((t0[j], t1[j]), lin), j


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_ciphertext_and_giant_tiles_of_bsgs(ctx, c):
    """c = 1, 2 and >= 3 take k_bsgs_inner<8, 1>, <4, 2> and <4, 4>: n_giant crosses ragged and full giant tiles of 4 and 8"""
    x = sweep_inputs()
    c0, c1 = x["c0"][:c], x["c1"][:c]
    for nb in (1, 3):
        for ng in (1, 3, 4, 5, 7, 8, 9):
            gb, gg = sweep_lists(nb, ng)
            o0, o1 = ctx.bfv_linear_transform_bsgs(SWEEP, c0, c1, gb, x["baby"][0][:nb], x["baby"][1][:nb], gg, x["giant"][0][:ng],
                                                   x["giant"][1][:ng], x["grid"][:ng, :nb], base_bits=SWEEP_W)
            for j in range(c):
                assert same((o0[j], o1[j]), sweep_bsgs_ref(nb, ng, j)), (nb, ng, j)


# ---- 3. many elements ----------------------------------------------------------------------------------------------------------

def test_six_hundred_elements(ctx):
    """N = 64, w = 32 (l = 2): 600 elements over all 64 odd g, a random key each; 600 2^62 > 2^64"""
    params, w, count = MANY, 32, 600
    rng = np.random.default_rng(600)
    elements = many_elements(count)
    gk0, gk1 = random_keys(rng, params, count, w)
    assert gk0.shape == (count, 2, 64) and range_bits(params, count, w) == 124
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    diag = plaintexts(rng, params, (count,))
    o0, o1 = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, diag, base_bits=w)
    for j in range(2):
        assert same((o0[j], o1[j]), ref_linear_transform(params, c0[j], c1[j], elements, gk0, gk1, w, diag)), j


def test_forty_by_forty_bsgs(ctx):
    params, w, side = MANY, 32, 40
    rng = np.random.default_rng(40)
    gb, gg = many_elements(side), many_elements(65)[-side:]   # g = 1 ... 79 and g = 51 ... 127, 1
    bk0, bk1 = random_keys(rng, params, side, w)
    hk0, hk1 = random_keys(rng, params, side, w)
    assert range_bits(params, side, w) == 120 and in_ranges(params, elements=gb + gg)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    diag = plaintexts(rng, params, (side, side))
    o0, o1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, gb, bk0, bk1, gg, hk0, hk1, diag, base_bits=w)
    for j in range(2):
        assert same((o0[j], o1[j]), ref_linear_transform_bsgs(params, c0[j], c1[j], gb, bk0, bk1, gg, hk0, hk1, w, diag)), j


# ---- 4. digit widths and moduli ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [Q63, Q62, QE])
def test_every_width_recomposes(ctx, q):
    """gk0_i = 2^(i w), gk1_i = 0: apply_galois and block k of apply_galois_many give (sigma_g(c0) + sigma_g(c1), 0)"""
    n = 64
    params = (n, q, 65537, 19)
    rng = np.random.default_rng(q % 1009)
    gs = [3, 2 * n - 1]
    for w in range(1, 33):
        l = relin_digits(q, w)
        gk0, gk1 = recomposition_key(n, q, w)
        c1 = width_rows(rng, n, q, w)
        c0 = residues(rng, params, c1.shape[0])
        assert any(int(x) >> ((l - 1) * w) for x in c1.reshape(-1)), w   # the top digit is non-zero somewhere
        m0, m1 = ctx.bfv_apply_galois_many(params, c0, c1, gs, np.stack([gk0, gk0]), np.stack([gk1, gk1]), base_bits=w)
        assert not m1.any(), w
        for k, g in enumerate(gs):
            a0, a1 = ctx.bfv_apply_galois(params, c0, c1, g, gk0, gk1, base_bits=w)
            assert not a1.any(), (w, g)
            for j in range(c1.shape[0]):
                want = sigma_sum(c0[j], c1[j], g, q)
                assert np.array_equal(a0[j], want), (w, g, j)
                assert np.array_equal(m0[k, j], want), (w, g, j)


WIDTHS = [(q, w) for q in (Q63, Q62) for w in (1, 7, 13, 21, 31, 32)] + [(Q29, 29), (Q29, 32)]


@pytest.mark.parametrize("q,w", WIDTHS)
def test_random_keys_at_odd_widths(ctx, q, w):
    """l w = bitlen(Q - 1) at (Q63, 21) and (Q62, 31); l = 1 at Q29"""
    n = 64
    params = (n, q, 65537, 19)
    rng = np.random.default_rng(q % 7919 + w)
    elements = [3, 1, 2 * n - 1, galois_element(n, 2)]
    gk0, gk1 = random_keys(rng, params, 4, w)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    c1[0, :4] = [q - 1, (1 << (relin_digits(q, w) - 1) * w), 0, q // 2]   # the top digit at its largest and smallest
    restate_four_calls(ctx, params, w, c0, c1, elements, gk0, gk1, plaintexts(rng, params, (4,)), 2, plaintexts(rng, params, (2, 2)))


TINY = [((8, 3, 2, 1), 1), ((8, 3, 2, 1), 2), ((8, 3, 2, 1), 32), ((16, Q62, 1 << 20, 19), 31), ((16, QE, 97, 19), 7)]


@pytest.mark.parametrize("params,w", TINY)
def test_tiny_and_odd_shaped_parameters(ctx, params, w):
    """at Q = 3 decryption is not expected to be right: the samples and the defining formulas are checked instead"""
    n, q, t, b = params
    rng = np.random.default_rng(q % 1000 + w)
    parties = PARTIES[:2]
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in parties]
    for k, ps in zip(keys, parties):
        assert same(k, ref_keygen_share(params, CRS, ps))
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]
    elements = [3, 1, 2 * n - 1, galois_element(n, 1)]
    seed = bytes([0x6d + w]) * 32
    gk0, gk1 = [], []
    for g in elements:
        assert same(ctx.bfv_galois_keygen(params, sks[0], g, seed=seed, base_bits=w), ref_galois_key(params, sks[0], seed, seed, g, w)), g
        shares = [ctx.bfv_galois_share(params, sk, CRS, ps, g, base_bits=w) for sk, ps in zip(sks, parties)]
        for sk, ps, got in zip(sks, parties, shares):
            assert same(got, ref_galois_key(params, sk, CRS, ps, g, w)), g
        gk0.append(ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])))
        gk1.append(shares[0][1])
        assert np.array_equal(gk0[-1], ref_aggregate(params, [s[0] for s in shares]))
    gk0, gk1 = np.array(gk0), np.array(gk1)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    restate_four_calls(ctx, params, w, c0, c1, elements, gk0, gk1, plaintexts(rng, params, (4,)), 2, plaintexts(rng, params, (2, 2)))
    # decryption shares and their combination, on arbitrary residues
    bound = min(1 << 10, (q // t - 1) // 2)
    d = [ctx.bfv_decrypt_share(params, sk, c1, seed=bytes([0x7b, i]) * 16, first_index=2, smudge_bound=bound) for i, sk in enumerate(sks)]
    for i, sk in enumerate(sks):
        assert np.array_equal(d[i], ref_decrypt_share(params, sk, c1, bytes([0x7b, i]) * 16, 2, bound)), i
    assert np.array_equal(ctx.bfv_decrypt_combine(params, c0, np.array(d)), ref_decrypt_combine(params, c0, d))
    if q > 3:   # a rotation of an encryption under the collective key opens to sigma_g(m)
        half = (t - 1) // 2   # below T/2 for even T, where T/2 and -T/2 are one class
        m = (rng.integers(-half, half + 1, size=(2, n)).astype(object) % q).astype(np.uint64)
        ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x6e" * 32)
        o0, o1 = ctx.bfv_apply_galois(params, ct["c0"], ct["c1"], 3, gk0[0], gk1[0], base_bits=w)
        d = [ctx.bfv_decrypt_share(params, sk, o1, seed=bytes([0x7c, i]) * 16, smudge_bound=bound) for i, sk in enumerate(sks)]
        got = ctx.bfv_decrypt_combine(params, o0, np.array(d))
        assert np.array_equal(got, ref_decrypt_combine(params, o0, d))
        for j in range(2):
            assert np.array_equal(got[j], sigma(m[j], 3, q)), j


@pytest.mark.parametrize("t", [2, Q60 - 2])
def test_plaintext_modulus_at_its_ends(ctx, t):
    """N = 8, w = 4: the rule gives 135 bits for one element at T = Q - 2; diagonals hold +-floor(T/2)"""
    params, w = (8, Q60, t, 19), 4
    n, q = params[0], params[1]
    rng = np.random.default_rng(t % 1000)
    elements = [3, 1, 15, 5]
    assert range_bits((8, Q60, Q60 - 2, 19), 1, w) == 135 and range_bits(params, 4, w) <= 150
    gk0, gk1 = random_keys(rng, params, 4, w)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    diag, bdiag = plaintexts(rng, params, (4,)), plaintexts(rng, params, (2, 2))
    diag[2], diag[3] = t // 2, q - t // 2   # whole diagonals at either end
    bdiag[1, 0], bdiag[0, 1] = t // 2, q - t // 2
    assert in_ranges(params, diags=[diag, bdiag])
    restate_four_calls(ctx, params, w, c0, c1, elements, gk0, gk1, diag, 2, bdiag)


def test_error_bound_1023_in_keys_and_shares(ctx):
    """B = 1023: the sampler's full table in the Galois keys, the key shares and both relinearization rounds, every error restated
    and within [-B, B]"""
    params, w = (64, Q60, 257, 1023), 16
    n, q, b = params[0], params[1], params[3]
    l = relin_digits(q, w)
    parties = PARTIES[:2]
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in parties]
    seen = []
    for k, ps in zip(keys, parties):
        assert same(k, ref_keygen_share(params, CRS, ps))
        seen.append(errors(q, neg(k[1], q), neg(ring_mul(k[2], k[0], q), q)))   # e = -(pk0 + a s)
    sks = [k[0] for k in keys]
    g, seed = galois_element(n, 3, True), b"\x6f" * 32
    for sk, got, crs, ps in ((sks[0], ctx.bfv_galois_keygen(params, sks[0], g, seed=seed, base_bits=w), seed, seed),
                             (sks[1], ctx.bfv_galois_share(params, sks[1], CRS, parties[1], g, base_bits=w), CRS, parties[1])):
        assert same(got, ref_galois_key(params, sk, crs, ps, g, w))
        ss = sigma(sk, g, q)
        for j in range(l):   # e_j = 2^(j w) sigma_g(s) - a_j s - r_j
            seen.append(errors(q, gadget(ss, j, w, q), neg(ring_mul(got[1][j], sk, q), q), neg(got[0][j], q)))
    r1 = [ctx.bfv_relin_share1(params, sk, CRS, ps, base_bits=w) for sk, ps in zip(sks, parties)]
    for sk, ps, (h0_i, h1_i) in zip(sks, parties, r1):
        assert same((h0_i, h1_i), ref_relin_share1(params, sk, CRS, ps, w))
        u = ternary(ps, 10, 0, n, q)
        for j in range(l):   # e0 = h0 + u a - 2^(j w) s and e1 = h1 - s a, a the CRS row (domain 7)
            a = uniform(CRS, 7, j, n, q)
            seen.append(errors(q, h0_i[j], ring_mul(u, a, q), neg(gadget(sk, j, w, q), q)))
            seen.append(errors(q, h1_i[j], neg(ring_mul(sk, a, q), q)))
    h0, h1 = (ref_aggregate(params, [x[k] for x in r1]) for k in (0, 1))
    for sk, ps in zip(sks, parties):
        got = ctx.bfv_relin_share2(params, sk, ps, h0, h1, base_bits=w)
        assert np.array_equal(got, ref_relin_share2(params, sk, ps, h0, h1, w))
        u_minus_s = add(ternary(ps, 10, 0, n, q), neg(sk, q), q=q)
        for j in range(l):   # e2 = r - s h0 - (u - s) h1
            seen.append(errors(q, got[j], neg(ring_mul(sk, h0[j], q), q), neg(ring_mul(u_minus_s, h1[j], q), q)))
    worst = max(max(abs(x) for x in e) for e in seen)
    print("B = 1023: %d error polynomials, max |e| = %d" % (len(seen), worst))
    assert worst <= b and all(any(e) for e in seen)


def test_smudging_bounds_at_their_ends(ctx):
    import zk_fhe_amd as zk
    # the largest bound: E = (floor(Q/T) - 1) / 2, about 2^61
    params = (64, Q63, 2, 19)
    n, q, t = params[0], params[1], params[2]
    bound = (q // t - 1) // 2
    assert bound.bit_length() == 61 and 2 * bound + 1 <= q // t < 2 * (bound + 1) + 1
    rng = np.random.default_rng(61)
    sk = ctx.bfv_keygen_share(params, CRS, PARTIES[0])[0]
    c1 = residues(rng, params, 3)
    d = ctx.bfv_decrypt_share(params, sk, c1, seed=b"\x7d" * 32, first_index=(1 << 32) - 1, smudge_bound=bound)
    assert np.array_equal(d, ref_decrypt_share(params, sk, c1, b"\x7d" * 32, (1 << 32) - 1, bound))
    noise = [x for j in range(3) for x in errors(q, d[j], neg(ring_mul(c1[j], sk, q), q))]
    assert max(abs(x) for x in noise) <= bound and max(abs(x) for x in noise) > bound // 2 and min(noise) < 0 < max(noise)
    with pytest.raises(zk.ZkfheError, match=r"2 smudge_bound \+ 1 must not exceed floor\(Q/T\)"):
        ctx.bfv_decrypt_share(params, sk, c1, seed=b"\x7d" * 32, smudge_bound=bound + 1)
    # the smallest: Q = 3, T = 2 leaves E = 0 only
    tiny = (8, 3, 2, 1)
    sk3 = ctx.bfv_keygen_share(tiny, CRS, PARTIES[0])[0]
    c3 = residues(rng, tiny, 2)
    d3 = ctx.bfv_decrypt_share(tiny, sk3, c3, seed=b"\x7e" * 32, smudge_bound=0)
    assert np.array_equal(d3, ref_decrypt_share(tiny, sk3, c3, b"\x7e" * 32, 0, 0))
    for j in range(2):
        assert np.array_equal(d3[j], ring_mul(c3[j], sk3, 3)), j
    with pytest.raises(zk.ZkfheError, match=r"2 smudge_bound \+ 1 must not exceed floor\(Q/T\)"):
        ctx.bfv_decrypt_share(tiny, sk3, c3, seed=b"\x7e" * 32, smudge_bound=1)
    # 1000 parties whose shares are all Q - 1: the sum passes 2^64 nine times over
    p8 = (8, Q63, 65537, 19)
    shares = np.full((1000, 2, 8), Q63 - 1, dtype=np.uint64)
    assert 1000 * (Q63 - 1) > 1 << 64
    agg = ctx.bfv_share_aggregate(p8, shares)
    assert np.array_equal(agg, ref_aggregate(p8, shares)) and set(int(x) for x in agg.reshape(-1)) == {Q63 - 1000}
    c0 = residues(rng, p8, 2)
    c0[0, :3] = [0, Q63 - 1, 1000]
    assert np.array_equal(ctx.bfv_decrypt_combine(p8, c0, shares), ref_decrypt_combine(p8, c0, shares))


# ---- 5. the range rule at its boundary ---------------------------------------------------------------------------------------------

BOUNDARY = [(1, 14, 15), (3, 13, 14)]   # (elements, the width with 150 bits, the width with 151)


def test_range_rule_accepts_150_bits_and_refuses_151(ctx):
    import zk_fhe_amd as zk
    params = EDGE
    n, q = params[0], params[1]
    z = np.zeros((1, n), dtype=np.uint64)
    bad = np.full((1, n), q, dtype=np.uint64)   # would be refused by the passes over the inputs, which come later
    g = [3, 15, 5]

    def flat(count, w, c0):
        keys = np.zeros((count, relin_digits(q, w), n), dtype=np.uint64)
        return ctx.bfv_linear_transform(params, c0, z, g[:count], keys, keys, np.zeros((count, n), np.uint64), base_bits=w)

    def bsgs(count, w, c0):
        keys, hk = np.zeros((count, relin_digits(q, w), n), dtype=np.uint64), np.zeros((1, relin_digits(q, w), n), dtype=np.uint64)
        return ctx.bfv_linear_transform_bsgs(params, c0, z, g[:count], keys, keys, [9], hk, hk, np.zeros((1, count, n), np.uint64), base_bits=w)

    ctx.prof_enable(True)
    try:
        for count, w_ok, w_no in BOUNDARY:
            assert (range_bits(params, count, w_ok), range_bits(params, count, w_no)) == (150, 151)
            for call in (flat, bsgs):
                for c0 in (z, bad):
                    with pytest.raises(zk.ZkfheError, match="needs 151 bits.*narrow base_bits, or split the element list"):
                        call(count, w_no, c0)
        for slot in range(5, 20):
            assert ctx.prof_read(slot)["launches"] == 0, slot
        for count, w_ok, w_no in BOUNDARY:
            for call in (flat, bsgs):
                o0, o1 = call(count, w_ok, z)
                assert not o0.any() and not o1.any()
                with pytest.raises(zk.ZkfheError, match="ciphertext coefficient is not below Q"):
                    call(count, w_ok, bad)
        assert ctx.prof_read(zk.PROF_BFV_LINEAR)["launches"] == 4 and ctx.prof_read(zk.PROF_BFV_BSGS_INNER)["launches"] == 2
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("params,w,elements", WORST)
def test_worst_case_magnitudes_on_the_accepted_side(ctx, params, w, elements):
    """|exact sum| near 2^146 of the 2^150 that the rule allows, in both signs (the host file proves the size of these inputs)"""
    n, q = params[0], params[1]
    c0, c1, gk0, gk1, diag = worst_case(params, w, elements)
    assert range_bits(params, len(elements), w) == 150
    hk = np.zeros((1,) + gk0.shape[1:], dtype=np.uint64)   # the key rows of the giant step g = 1 are not read
    for d in (diag, negated(params, diag)):
        want = ref_linear_transform(params, c0, c1, elements, gk0, gk1, w, d)
        o0, o1 = ctx.bfv_linear_transform(params, c0, c1, elements, gk0, gk1, d, base_bits=w)
        assert same((o0[0], o1[0]), want)
        b0, b1 = ctx.bfv_linear_transform_bsgs(params, c0, c1, elements, gk0, gk1, [1], hk, hk, d[None], base_bits=w)
        assert same((b0[0], b1[0]), want)
