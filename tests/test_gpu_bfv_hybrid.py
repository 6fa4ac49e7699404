"""Hybrid key switching on the GPU (bfv_hybrid.hip, bfv_evk.hip and the hybrid epilogues of bfv_eval.hip and bfv_pack.hip): the keys
from zkfhe_bfv_*_keygen_hybrid against the restatement from their seeds, and zkfhe_bfv_cts_mul_evk, _apply_galois_evk, _slot_sum, _dot
and _pack with a hybrid key set bit for bit against the Python big-integer restatement of tests/test_bfv_hybrid_host.py, at the small
shapes for every digit width and kind of special modulus and at the k = 13 parameters, each at a count that takes the digit-parallel
key switch and one above Context.bfv_evk_wide_max; the rounding at exact ties for an even and an odd P; the edge of the bound; a batch
across two chunks; a committee's aggregated key; the noise bound; the refusals of creation in their order.
At N = 32768 one restated ciphertext costs about 5 s (apply_galois) or 10 s (mul) of big-integer products, so the two chunk-crossing
tests restate the first ciphertext of the second chunk and hold the rest against the same call on each chunk alone.
Run on the MI355X box: pytest -m gpu."""
import math

import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60, Q63, circ, deg, kron_negacyclic, relin_digits
from tests.test_bfv_galois_host import sigma, slot_sum_elements
from tests.test_bfv_hybrid_host import (K13, P5, P30, bound_holds, lift, max_p, ref_apply_galois_hybrid, ref_dot_hybrid, ref_hybrid_key,
                                        ref_mul_hybrid, ref_pack_hybrid, ref_slot_sum_hybrid, switch_noise_bound)
from tests.test_bfv_pack_host import expected_plain, pack_elements
from tests.test_bfv_threshold_host import ref_decrypt
from tests.test_gpu_bfv_resident import pair, same

pytestmark = pytest.mark.gpu
S8, S16, S32 = (8, Q29, 7, 19), (16, Q60, 97, 19), (32, 1 << 16, 7, 19)
BIG, CROSS = (32768, Q60, 65537, 19), 65   # chunk_polys(N) = 64
KEY_SEED, RLK_SEED, GK_SEED, ENC_SEED = b"\x91" * 32, b"\x92" * 32, b"\x93" * 32, b"\x94" * 32


def coprime_below(top, q):
    while math.gcd(top, q) != 1:
        top -= 1
    return top


def moduli(params, w):
    """a 30-bit odd P, 2^20 where Q is odd, an odd P just below 2^63 where the bound allows, the largest admissible P coprime to Q"""
    q, top = params[1], max_p(params, w)
    out = [P30] + ([1 << 20] if q & 1 else []) + ([Q63] if Q63 <= top else []) + [coprime_below(top, q)]
    assert all(bound_holds(params, w, p) and math.gcd(p, q) == 1 for p in out)
    return list(dict.fromkeys(out))


SMALL = [(params, w, p) for params in (S8, S16, S32) for w in (4, 8, 16) for p in moduli(params, w)]
AT_K13 = [(K13, 8, p) for p in moduli(K13, 8) if p not in (1 << 20, Q63)]
ids = lambda c: "N%d-w%d-P%d" % (c[0][0], c[1], c[2])  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def stack(keys, elements):
    return tuple(np.array([keys[g][j] for g in elements]) for j in range(4))


class Material:
    """one secret key with its hybrid relinearization key and the hybrid Galois keys of the slot-sum and pack elements, as host planes
    and as a key set; fixed seeds"""

    def __init__(self, ctx, params, w, p):
        n = params[0]
        self.params, self.w, self.p = params, w, p
        self.sk, self.pk0, self.pk1 = ctx.bfv_fhe_keypair(params, KEY_SEED)
        self.rlk = ctx.bfv_relin_keygen_hybrid(params, p, self.sk, RLK_SEED, base_bits=w)
        self.elements = sorted(set(slot_sum_elements(n)) | (set(pack_elements(n)) if params[1] & 1 else set()))
        self.gk = {g: ctx.bfv_galois_keygen_hybrid(params, p, self.sk, g, seed=GK_SEED, base_bits=w) for g in self.elements}
        self.evk = ctx.bfv_evk_hybrid(params, p, w, rlk=self.rlk, elements=self.elements, gk=stack(self.gk, self.elements))


@pytest.fixture(scope="module")
def material(ctx):
    made = {}

    def get(case):
        if case not in made:
            made[case] = Material(ctx, *case)
        return made[case]

    yield get
    for m in made.values():
        m.evk.close()


def counts(ctx, params, w):
    """a count that goes the digit-parallel way (where l >= 2) and the first count past it"""
    return sorted({1, 3, ctx.bfv_evk_wide_max(params, w) + 1})


def picks(ctx, case):
    """(count, the ciphertexts of it that are restated): everything at the small shapes; at k = 13 at most 8 in all"""
    params, w, _ = case
    if params[0] <= 32:
        return [(c, range(c)) for c in counts(ctx, params, w)]
    above = ctx.bfv_evk_wide_max(params, w) + 1
    return [(2, range(2)), (above, (0, above - 1))]


def equal(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 1. the keys -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SMALL + AT_K13, ids=ids)
def test_keys_match_the_restatement(ctx, material, case):
    import zk_fhe_amd as zk
    params, w, p = case
    m = material(case)
    assert all(np.array_equal(a, b) for a, b in zip(m.rlk, ref_hybrid_key(params, p, m.sk, RLK_SEED, RLK_SEED, None, w)))
    for g in m.elements if params[0] <= 32 else m.elements[:2]:
        assert all(np.array_equal(a, b) for a, b in zip(m.gk[g], ref_hybrid_key(params, p, m.sk, GK_SEED, GK_SEED, g, w))), g
    g = m.elements[0]
    share = ctx.bfv_galois_share_hybrid(params, p, m.sk, GK_SEED, GK_SEED, g, base_bits=w)
    assert all(np.array_equal(a, b) for a, b in zip(share, m.gk[g]))
    other = ctx.bfv_galois_share_hybrid(params, p, m.sk, GK_SEED, RLK_SEED, g, base_bits=w)   # the CRS alone decides a
    assert np.array_equal(other[1], share[1]) and np.array_equal(other[3], share[3]) and not np.array_equal(other[0], share[0])
    assert all(np.array_equal(a, b) for a, b in zip(other, ref_hybrid_key(params, p, m.sk, GK_SEED, RLK_SEED, g, w)))
    assert m.evk.special_modulus == p
    assert m.evk.info() == {"params": params, "base_bits": w, "has_relin": True, "elements": m.elements,
                            "device_bytes": zk.bfv_evk_bytes(params, w, True, len(m.elements))}


# ---- 2. every call against the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SMALL + AT_K13, ids=ids)
def test_mul_evk(ctx, material, case):
    params, w, p = case
    m = material(case)
    for count, which in picks(ctx, case):
        rng = np.random.default_rng(300 + count)
        a, b = pair(rng, params, count), pair(rng, params, count)
        with ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y, x.mul_evk(y, m.evk) as out:
            got = out.download()
        for i in which:
            assert equal((got[0][i], got[1][i]), ref_mul_hybrid(params, p, a[0][i], a[1][i], b[0][i], b[1][i], m.rlk, w)), (count, i)


@pytest.mark.parametrize("case", SMALL + AT_K13, ids=ids)
def test_dot(ctx, material, case):
    params, w, p = case
    m = material(case)
    n, n_terms = params[0], 2
    for n_groups, which in picks(ctx, case):
        rng = np.random.default_rng(310 + n_groups)
        a, b = pair(rng, params, n_groups * n_terms), pair(rng, params, n_groups * n_terms)
        with ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y, x.dot(y, n_terms, m.evk) as out:
            got = out.download()
        A, B = [v.reshape(n_groups, n_terms, n) for v in a], [v.reshape(n_groups, n_terms, n) for v in b]
        for i in which:
            assert equal((got[0][i], got[1][i]), ref_dot_hybrid(params, p, A[0][i], A[1][i], B[0][i], B[1][i], m.rlk, w)), (n_groups, i)


@pytest.mark.parametrize("case", SMALL + AT_K13, ids=ids)
def test_apply_galois_evk(ctx, material, case):
    params, w, p = case
    m = material(case)
    for count, which in picks(ctx, case):
        a = pair(np.random.default_rng(320 + count), params, count)
        for g in (5, 2 * params[0] - 1):
            with ctx.bfv_cts(params, *a) as x:
                assert x.apply_galois_evk(g, m.evk, out=x) is x   # the destination is the source
                got = x.download()
            for i in which:
                assert equal((got[0][i], got[1][i]), ref_apply_galois_hybrid(params, p, a[0][i], a[1][i], g, m.gk[g], w)), (count, g, i)


@pytest.mark.parametrize("case", SMALL + AT_K13, ids=ids)
def test_slot_sum(ctx, material, case):
    params, w, p = case
    m = material(case)
    gks = [m.gk[g] for g in slot_sum_elements(params[0])]
    for count, which in picks(ctx, case):
        a = pair(np.random.default_rng(330 + count), params, count)
        with ctx.bfv_cts(params, *a) as x, x.slot_sum(m.evk) as out:
            got = out.download()
        for i in list(which)[:1 if params[0] > 32 else None]:
            assert equal((got[0][i], got[1][i]), ref_slot_sum_hybrid(params, p, a[0][i], a[1][i], gks, w)), (count, i)


@pytest.mark.parametrize("case", [c for c in SMALL if c[0][1] & 1], ids=ids)
def test_pack(ctx, material, case):
    """n = 1, a non-power of two and N inputs; one group (every level digit-parallel where l >= 2) and as many groups as put the
    first levels above the bound and the last ones below it"""
    params, w, p = case
    m = material(case)
    n_ring = params[0]
    gks = [m.gk[g] for g in pack_elements(n_ring)]
    for n in (1, 3, n_ring):
        for n_groups in (1, 2 * ctx.bfv_evk_wide_max(params, w) // n + 2):
            rng = np.random.default_rng(340 + n + n_groups)
            a = pair(rng, params, n_groups * n)
            pos = rng.integers(0, n_ring, size=(n_groups, n), dtype=np.uint64)
            with ctx.bfv_cts(params, *a) as x, x.pack(n, m.evk, pos=pos.reshape(-1)) as out:
                assert out.info()["n"] == n_groups
                got = out.download()
            for i in range(n_groups):
                want = ref_pack_hybrid(params, p, a[0][i * n:(i + 1) * n], a[1][i * n:(i + 1) * n], [int(v) for v in pos[i]], gks, w)
                assert equal((got[0][i], got[1][i]), want), (n, n_groups, i)


@pytest.mark.parametrize("case", AT_K13, ids=ids)
def test_pack_and_noise_at_k13(ctx, material, case):
    """8 fresh ciphertexts: the pack equals the restatement and decrypts to the chosen coefficients; one apply_galois adds at most
    ceil(l N (2^w - 1) B / P) + (N + 1) / 2 to the noise"""
    params, w, p = case
    m = material(case)
    n_ring, q, t = params[0], params[1], params[2]
    rng = np.random.default_rng(350)
    ms = rng.integers(0, t // 2 + 1, size=(8, n_ring), dtype=np.uint64)
    ms = np.where(rng.integers(0, 2, size=ms.shape).astype(bool) & (ms > 0), q - ms, ms)
    enc = ctx.bfv_encrypt(params, m.pk0, m.pk1, ms, seed=ENC_SEED)
    pos = [int(v) for v in rng.integers(0, n_ring, size=8)]
    with ctx.bfv_cts(params, enc["c0"], enc["c1"]) as x:
        with x.pack(8, m.evk, pos=np.array(pos, dtype=np.uint64)) as out:
            got = out.download()
        with x.apply_galois_evk(5, m.evk) as out:
            rot = out.download()
    want = ref_pack_hybrid(params, p, enc["c0"], enc["c1"], pos, [m.gk[g] for g in pack_elements(n_ring)], w)
    assert equal((got[0][0], got[1][0]), want)
    assert np.array_equal(ctx.bfv_decrypt(params, m.sk, *got)[0], expected_plain(params, ms, pos))
    before, after = ctx.bfv_noise(params, m.sk, enc["c0"], enc["c1"]), ctx.bfv_noise(params, m.sk, *rot)
    bound = switch_noise_bound(params, w, p)
    print("k = 13, w = %d, P = %d: noise in %s, out %s, bound on the increase %d" % (w, p, list(before), list(after), bound))
    assert all(int(o) <= int(i) + bound for i, o in zip(before, after))
    assert np.array_equal(ctx.bfv_decrypt(params, m.sk, *rot), np.array([sigma(v, 5, q) for v in ms]))


# ---- 3. rounding and the edge of the bound ---------------------------------------------------------------------------------------

def one_key(params, w, p, k0_rows):
    """the planes of a key whose K0 rows are the given integer polynomials (degree order, below Q P) and whose K1 is zero"""
    q = params[1]
    zero = np.zeros((len(k0_rows), params[0]), dtype=np.uint64)
    return np.array([circ(r, q) for r in k0_rows]), zero, np.array([circ(r, p) for r in k0_rows]), zero


@pytest.mark.parametrize("p", [1 << 20, P30], ids=["even", "odd"])
@pytest.mark.parametrize("by_x", [False, True], ids=["constant", "times_x"])
def test_rounding_at_ties(ctx, p, by_x):
    """K0_0 = k or k x and a source with digits at degrees 0, 1 and N - 1: X holds a k and, through x^N = -1, -a k.  Even P: k = P / 2
    and odd a make every such coefficient an exact tie; odd P: k = (P +- 1) / 2 puts X half a step on either side of one."""
    params, w = S8, 8
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    for k in ([p // 2] if p % 2 == 0 else [(p - 1) // 2, (p + 1) // 2]):
        row = [0] * n
        row[1 if by_x else 0] = k
        key = one_key(params, w, p, [row] + [[0] * n] * (l - 1))
        src = [1, 3] + [0] * (n - 3) + [5]   # degree order
        c0, c1 = np.zeros((1, n), dtype=np.uint64), circ(src, q)[None]
        with ctx.bfv_evk_hybrid(params, p, w, elements=[1], gk=tuple(v[None] for v in key)) as evk, ctx.bfv_cts(params, c0, c1) as x, \
                x.apply_galois_evk(1, evk) as out:
            got = out.download()
        xs = kron_negacyclic([(src, row)], n)
        assert sorted(set(xs)) == sorted({0, k, 3 * k, 5 * k} if not by_x else {0, k, 3 * k, -5 * k})
        want = circ([(2 * v + p) // (2 * p) for v in xs], q)   # the floor definition on the integers themselves
        assert np.array_equal(got[0][0], want) and not got[1].any()
        assert equal((got[0][0], got[1][0]), ref_apply_galois_hybrid(params, p, c0[0], c1[0], 1, key, w))
        if by_x and p % 2 == 0:
            assert (2 * -5 * k + p) // (2 * p) == -2 and deg(want)[0] == q - 2   # -2.5 rounds upward, to -2


@pytest.mark.parametrize("params,w", [(S32, 8), ((4096, Q60, 65537, 19), 32)], ids=["N32-w8", "N4096-w32"])
def test_the_edge_of_the_bound(ctx, params, w):
    """Every source coefficient Q - 1, every key word (Q - 1, P - 1), P the largest admissible odd value.  Q = 2^16, w = 8: every digit
    is 255 and the top coefficient of X is exactly l N 255 (Q P - 1).  N = 4096, 60-bit Q, w = 32: zkfhe_bfv_hybrid_max_p is below
    2^63 and the top coefficient lies above a quarter of P5, within a factor of two of the bound."""
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    p = max_p(params, w)
    p -= 1 - p % 2
    assert bound_holds(params, w, p)
    key = tuple(np.full((l, n), v, dtype=np.uint64) for v in (q - 1, q - 1, p - 1, p - 1))
    assert lift(key[0][0], key[2][0], q, p) == [q * p - 1] * n
    c = np.full((1, n), q - 1, dtype=np.uint64)
    digits = [((q - 1) >> (i * w)) & ((1 << w) - 1) for i in range(l)]
    top = kron_negacyclic([([d] * n, [q * p - 1] * n) for d in digits], n)[n - 1]
    assert top == sum(digits) * n * (q * p - 1) <= P5 // 2
    if n == 32:
        assert digits == [255, 255] and top == l * n * 255 * (q * p - 1)
    else:
        assert p < 1 << 62 and not bound_holds(params, w, max_p(params, w) + 1) and top > P5 // 4
    with ctx.bfv_evk_hybrid(params, p, w, elements=[1], gk=tuple(v[None] for v in key)) as evk, ctx.bfv_cts(params, c, c) as x, \
            x.apply_galois_evk(1, evk) as out:
        got = out.download()
    assert equal((got[0][0], got[1][0]), ref_apply_galois_hybrid(params, p, c[0], c[0], 1, key, w))


# ---- 4. across two chunks --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(365)
    a, b = pair(rng, BIG, CROSS), pair(rng, BIG, CROSS)
    for x in a + b:
        x.setflags(write=False)
    return a, b


def halves(ctx, srcs, call):
    """call on the first 64 ciphertexts and on the 65th, each a batch of its own"""
    out = []
    for lo, hi in ((0, CROSS - 1), (CROSS - 1, CROSS)):
        batches = [ctx.bfv_cts(BIG, s[0][lo:hi], s[1][lo:hi]) for s in srcs]
        try:
            with call(*batches) as o:
                out.append(o.download())
        finally:
            for b in batches:
                b.close()
    return np.concatenate([out[0][0], out[1][0]]), np.concatenate([out[0][1], out[1][1]])


def test_mul_evk_across_a_chunk(ctx, big):
    a, b = big
    w, p, i = 32, P30, CROSS - 1
    sk = ctx.bfv_fhe_keypair(BIG, KEY_SEED)[0]
    rlk = ctx.bfv_relin_keygen_hybrid(BIG, p, sk, RLK_SEED, base_bits=w)
    with ctx.bfv_evk_hybrid(BIG, p, w, rlk=rlk) as evk:
        with ctx.bfv_cts(BIG, *a) as x, ctx.bfv_cts(BIG, *b) as y:
            assert x.mul_evk(y, evk, out=x) is x and same(y, b)
            got = x.download()
        assert equal(got, halves(ctx, [a, b], lambda u, v: u.mul_evk(v, evk)))
    assert equal((got[0][i], got[1][i]), ref_mul_hybrid(BIG, p, a[0][i], a[1][i], b[0][i], b[1][i], rlk, w))


def test_apply_galois_evk_across_a_chunk(ctx, big):
    a, _ = big
    w, p, g, i = 32, P30, 5, CROSS - 1
    sk = ctx.bfv_fhe_keypair(BIG, KEY_SEED)[0]
    gk = ctx.bfv_galois_keygen_hybrid(BIG, p, sk, g, seed=GK_SEED, base_bits=w)
    with ctx.bfv_evk_hybrid(BIG, p, w, elements=[g], gk=tuple(v[None] for v in gk)) as evk:
        with ctx.bfv_cts(BIG, *a) as x:
            assert x.apply_galois_evk(g, evk, out=x) is x
            got = x.download()
        assert equal(got, halves(ctx, [a], lambda u: u.apply_galois_evk(g, evk)))
    assert equal((got[0][i], got[1][i]), ref_apply_galois_hybrid(BIG, p, a[0][i], a[1][i], g, gk, w))


# ---- 5. a committee's key --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [P30, coprime_below(max_p(S16, 8), Q60)], ids=["P30", "max"])
def test_three_party_aggregate_decrypts_rotations(ctx, p):
    params, w = S16, 8
    n, q, t = params[0], params[1], params[2]
    crs, seeds = b"\xa0" * 32, [bytes([0xa1 + i]) * 32 for i in range(3)]
    parts = [ctx.bfv_keygen_share(params, crs, s) for s in seeds]
    sks = [x[0] for x in parts]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([x[1] for x in parts])), parts[0][2]
    s = np.array([sum(int(v) - q if int(v) > q // 2 else int(v) for v in col) % q for col in zip(*sks)], dtype=np.uint64)   # not ternary
    rng = np.random.default_rng(370)
    ms = rng.integers(0, t // 2 + 1, size=(3, n), dtype=np.uint64)
    enc = ctx.bfv_encrypt(params, pk0, pk1, ms, seed=ENC_SEED)
    elements = [5, 2 * n - 1]
    planes = []
    for g in elements:
        shares = [ctx.bfv_galois_share_hybrid(params, p, sk, crs, seed, g, base_bits=w) for sk, seed in zip(sks, seeds)]
        assert all(np.array_equal(x[1], shares[0][1]) and np.array_equal(x[3], shares[0][3]) for x in shares)
        planes.append((ctx.bfv_share_aggregate(params, np.array([x[0] for x in shares])), shares[0][1],
                       ctx.bfv_share_aggregate((n, p, 2, 1), np.array([x[2] for x in shares])), shares[0][3]))   # the p-planes mod P
    gk = tuple(np.array([k[j] for k in planes]) for j in range(4))
    with ctx.bfv_evk_hybrid(params, p, w, elements=elements, gk=gk) as evk, ctx.bfv_cts(params, enc["c0"], enc["c1"]) as x:
        for g, key in zip(elements, planes):
            with x.apply_galois_evk(g, evk) as out:
                got = out.download()
            assert equal((got[0][0], got[1][0]), ref_apply_galois_hybrid(params, p, enc["c0"][0], enc["c1"][0], g, key, w))
            assert np.array_equal(ref_decrypt(params, s, *got), np.array([sigma(v, g, q) for v in ms]))


# ---- 6. creation -----------------------------------------------------------------------------------------------------------------

def test_an_ordinary_set_keeps_its_bits_and_has_special_modulus_one(ctx):
    params, w = S8, 8
    sk = ctx.bfv_fhe_keypair(params, KEY_SEED)[0]
    rlk = ctx.bfv_relin_keygen(params, sk, RLK_SEED, base_bits=w)
    gk0, gk1 = ctx.bfv_galois_keygen(params, sk, 5, seed=GK_SEED, base_bits=w)
    rng = np.random.default_rng(380)
    a, b = pair(rng, params, 3), pair(rng, params, 3)
    with ctx.bfv_evk(params, w, rlk, [5], gk0[None], gk1[None]) as evk, ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y:
        assert evk.special_modulus == 1
        with x.mul_evk(y, evk) as out:
            assert same(out, ctx.bfv_mul(params, *a, *b, *rlk, base_bits=w))
        with x.apply_galois_evk(5, evk) as out:
            assert same(out, ctx.bfv_apply_galois(params, *a, 5, gk0, gk1, base_bits=w))


def test_refusals_of_creation_in_their_order(ctx):
    import zk_fhe_amd as zk
    fn = "bfv_evk_create_hybrid: "
    params, w = (4096, Q60, 65537, 19), 32   # zkfhe_bfv_hybrid_max_p is below 2^63 here
    n, q = params[0], params[1]
    l, limit = relin_digits(q, w), max_p(params, w)
    assert limit < (1 << 63) - 1 and zk.bfv_hybrid_max_p(params, w) == limit
    p = coprime_below(limit, q)
    zero = np.zeros((l, n), dtype=np.uint64)
    ok, bad_q, bad_p = (zero,) * 4, (zero, np.full((l, n), q, dtype=np.uint64), zero, zero), (zero, zero, np.full((l, n), p, dtype=np.uint64), zero)
    both = (bad_q[1], zero, bad_p[2], zero)
    two = tuple(np.array([v, v]) for v in ok)

    def refused(text, p, w, rlk=None, elements=(), gk=None, params=params):
        with pytest.raises(zk.ZkfheError) as err:
            ctx.bfv_evk_hybrid(params, p, w, rlk=rlk, elements=elements, gk=gk)
        assert str(err.value).endswith(fn + text) or fn + text in str(err.value), str(err.value)

    refused("neither a relinearization key nor a Galois key", 1, 0)                       # 1. nothing to hold, before everything
    with pytest.raises(zk.ZkfheError, match="bfv params"):                                # 2. the parameters, before P
        ctx.bfv_evk_hybrid((n, q, q, 19), 1, 0, rlk=ok)
    refused("base_bits must be in [1, 32]", 1, 0, rlk=ok)                                 # 2. base_bits, before P
    for bad in (0, 1, 1 << 63):
        refused("P must satisfy 2 <= P < 2^63", bad, w, rlk=both, elements=[6, 6], gk=two)                       # 3. before g
    refused("P and Q must be coprime", 9, w, rlk=ok, elements=[6, 6], gk=two, params=(n, 3 << 40, 65537, 19))    # 4. before g (l = 2 too)
    refused("P and Q must be coprime", q, w, rlk=both, elements=[6, 6], gk=two)                                  # 4. Q > the limit
    refused("P is above the limit %d of zkfhe_bfv_hybrid_max_p" % limit, limit + 1, w, rlk=both, elements=[6, 6], gk=two)   # 5. before g
    refused("the Galois element g must be odd and below 2N", p, w, rlk=both, elements=[5, 6], gk=two)            # 6. before the planes
    refused("the Galois element 5 is repeated", p, w, rlk=both, elements=[5, 5], gk=two)
    refused("a relinearization-key coefficient is not below Q", p, w, rlk=both)                                  # 7. before the p-planes
    refused("a Galois-key coefficient is not below Q", p, w, rlk=ok, elements=[5], gk=tuple(v[None] for v in both))
    refused("a relinearization-key p-plane coefficient is not below P", p, w, rlk=bad_p)                         # 8.
    refused("a Galois-key p-plane coefficient is not below P", p, w, elements=[5], gk=tuple(v[None] for v in bad_p))
    edge = (np.full((l, n), q - 1, dtype=np.uint64), zero, np.full((l, n), p - 1, dtype=np.uint64), zero)        # Q - 1, P - 1 are residues
    with ctx.bfv_evk_hybrid(params, p, w, rlk=edge) as evk:
        assert evk.special_modulus == p and evk.info()["has_relin"]
    for name, args in (("bfv_relin_keygen_hybrid", ()), ("bfv_galois_keygen_hybrid", (5,))):
        with pytest.raises(zk.ZkfheError, match=name + ": P is above the limit"):
            getattr(ctx, name)(params, limit + 1, np.zeros(n, dtype=np.uint64), *args, seed=KEY_SEED, base_bits=w)
    with pytest.raises(zk.ZkfheError, match="bfv_galois_share_hybrid: P and Q must be coprime"):
        ctx.bfv_galois_share_hybrid(params, q, np.zeros(n, dtype=np.uint64), KEY_SEED, KEY_SEED, 5, base_bits=w)
    with pytest.raises(zk.ZkfheError, match="bfv_relin_keygen_hybrid: B must be below Q / 2"):   # e is read back centred from e mod Q
        ctx.bfv_relin_keygen_hybrid((8, 37, 7, 19), P30, np.zeros(8, dtype=np.uint64), seed=KEY_SEED, base_bits=8)
