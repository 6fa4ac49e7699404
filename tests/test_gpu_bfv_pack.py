"""Ring packing on the GPU (bfv_pack.hip; zkfhe.h "Ring packing"): the monomial product against its restatement and against
bfv_mul_plain by +-x^k; bfv_pack bit for bit against the restated pack of tests/test_bfv_pack_host.py and decrypted to the expected
placement, with one secret key and with the collective keys of three parties; the batch call against the host-array call; the fused
call against the composition by hand from the existing batch calls, level by level, across chunk_polys and through the root stack;
the launches per profiling slot; and the refusals in their order, each leaving dst as it was.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60
from tests.test_bfv_pack_host import expected_plain, list_of_n, monomial, padded, pack_elements, ref_pack
from tests.test_gpu_bfv_eval import random_residues
from tests.test_gpu_bfv_resident import check_call, pair, same

pytestmark = pytest.mark.gpu
P8 = (8, Q29, 7, 19)
P16 = (16, Q60, 97, 19)
P32 = (32, Q29, 7, 19)
K13 = (1024, Q29, 7, 19)        # the k = 13 parameters: T does not batch
P4096 = (4096, Q60, 65537, 19)  # chunk_polys(N) = 512
BIG = (32768, Q60, 65537, 19)   # chunk_polys(N) = 64; the key switch's LDS is 128 KiB
RNS_NTT = 6
CRS = b"\xc5" * 32
PARTIES = [bytes([0x48 + i]) * 32 for i in range(3)]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


class PackKeys:
    """one secret key, its public key and the Galois keys of the pack elements, as host arrays and as a key set; fixed seeds"""

    def __init__(self, ctx, params, w):
        self.params, self.w = params, w
        self.sk, self.pk0, self.pk1 = ctx.bfv_fhe_keypair(params, b"\x81" * 32)
        self.elements = pack_elements(params[0])
        keys = [ctx.bfv_galois_keygen(params, self.sk, g, seed=b"\x82" * 32, base_bits=w) for g in self.elements]
        self.gk0, self.gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
        self.evk = ctx.bfv_evk(params, w, None, self.elements, self.gk0, self.gk1)


@pytest.fixture(scope="module")
def keysets(ctx):
    made = {}

    def get(params, w):
        if (params, w) not in made:
            made[(params, w)] = PackKeys(ctx, params, w)
        return made[(params, w)]

    yield get
    for k in made.values():
        k.evk.close()


def messages(rng, params, shape):
    """plaintexts with coefficients in [-T/2, T/2], as residues mod Q"""
    q, t = params[1], params[2]
    v = rng.integers(-(t // 2), t // 2 + 1, size=shape + (params[0],))
    return np.where(v < 0, v + q, v).astype(np.uint64)


def groups_of(rng, params, n_groups, n):
    """n_groups n ciphertexts of random residues, (n_groups, n, N) each"""
    shape = (n_groups, n, params[0])
    return random_residues(rng, shape, params[1]), random_residues(rng, shape, params[1])


# ---- 1. the monomial product -------------------------------------------------------------------------------------------------------

def exponents(n_ring):
    return [0, 1, n_ring - 1, n_ring, n_ring + 1, 2 * n_ring - 1]


@pytest.mark.parametrize("params", [P8, K13], ids=["P8", "K13"])
def test_mul_monomial_is_the_restatement_and_mul_plain_by_a_signed_monomial(ctx, params):
    n_ring, q = params[0], params[1]
    ks = exponents(n_ring)
    a = pair(np.random.default_rng(400 + n_ring), params, len(ks))
    per = ctx.bfv_mul_monomial(params, *a, ks)   # one exponent per ciphertext
    for i, k in enumerate(ks):
        want = monomial(a[0][i], k, q), monomial(a[1][i], k, q)
        assert np.array_equal(per[0][i], want[0]) and np.array_equal(per[1][i], want[1]), k
        shared = ctx.bfv_mul_monomial(params, a[0][:2], a[1][:2], k)   # one exponent for all
        assert np.array_equal(shared[0][0], monomial(a[0][0], k, q)) and np.array_equal(shared[1][1], monomial(a[1][1], k, q)), k
        m = np.zeros(n_ring, dtype=np.uint64)   # the plaintext x^k, or -x^(k - N)
        m[n_ring - 1 - k % n_ring] = 1 if k < n_ring else q - 1
        plain = ctx.bfv_mul_plain(params, a[0][i], a[1][i], m)
        assert np.array_equal(plain[0][0], per[0][i]) and np.array_equal(plain[1][0], per[1][i]), k


@pytest.mark.parametrize("params", [P8, K13], ids=["P8", "K13"])
def test_batch_mul_monomial_is_the_host_array_call(ctx, params):
    n_ring = params[0]
    ks = exponents(n_ring)
    a = pair(np.random.default_rng(410 + n_ring), params, len(ks))
    check_call(ctx, params, [a], lambda c0, c1: ctx.bfv_mul_monomial(params, c0, c1, ks), lambda x, out: x.mul_monomial(ks, out=out))
    check_call(ctx, params, [a], lambda c0, c1: ctx.bfv_mul_monomial(params, c0, c1, n_ring + 1), lambda x, out: x.mul_monomial(n_ring + 1, out=out))


# ---- 2. bfv_pack against the restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("with_pos", [False, True], ids=["pos-none", "pos-random"])
@pytest.mark.parametrize("params,w,decrypts", [(P8, 8, True), (P16, 16, True), (P32, 4, True), (P8, 32, False)],
                         ids=["N8-w8", "N16-w16", "N32-w4", "N8-w32"])
def test_pack_is_the_restatement_and_decrypts_to_the_placement(ctx, keysets, params, w, decrypts, with_pos, n_groups):
    """w = 32 (l = 1) is held to the bits only: the noise bound does not cover it"""
    n_ring = params[0]
    k = keysets(params, w)
    rng = np.random.default_rng(420 + n_ring + w)
    for n in list_of_n(n_ring):
        m = messages(rng, params, (n_groups, n))
        ct = ctx.bfv_encrypt(params, k.pk0, k.pk1, m.reshape(-1, n_ring), b"\x83" * 32)
        c0, c1 = ct["c0"].reshape(m.shape), ct["c1"].reshape(m.shape)
        pos = rng.integers(0, n_ring, size=(n_groups, n), dtype=np.uint64) if with_pos else None
        got = ctx.bfv_pack(params, c0 if n_groups > 1 else c0[0], c1 if n_groups > 1 else c1[0], k.gk0, k.gk1, pos=pos, base_bits=w)
        assert got[0].shape == (n_groups, n_ring)
        for g in range(n_groups):
            want = ref_pack(params, c0[g], c1[g], None if pos is None else pos[g], k.gk0, k.gk1, w)
            assert np.array_equal(got[0][g], want[0]) and np.array_equal(got[1][g], want[1]), (n, g)
        if decrypts:
            plain = ctx.bfv_decrypt(params, k.sk, *got)
            for g in range(n_groups):
                assert np.array_equal(plain[g], expected_plain(params, m[g], None if pos is None else pos[g])), (n, g)


def test_three_parties_pack_and_open_with_one_round_of_shares(ctx):
    params, w = P8, 8
    n_ring = params[0]
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES]
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]
    gk0, gk1 = [], []
    for g in pack_elements(n_ring):
        shares = [ctx.bfv_galois_share(params, sk, CRS, ps, g, base_bits=w) for sk, ps in zip(sks, PARTIES)]
        gk0.append(ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])))
        gk1.append(shares[0][1])
    gk0, gk1 = np.array(gk0), np.array(gk1)
    rng = np.random.default_rng(430)
    n = 5
    m = messages(rng, params, (n,))
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x84" * 32)
    pos = rng.integers(0, n_ring, size=n, dtype=np.uint64)
    o0, o1 = ctx.bfv_pack(params, ct["c0"], ct["c1"], gk0, gk1, pos=pos, base_bits=w)
    want = ref_pack(params, ct["c0"], ct["c1"], pos, gk0, gk1, w)
    assert np.array_equal(o0[0], want[0]) and np.array_equal(o1[0], want[1])
    shares = [ctx.bfv_decrypt_share(params, sk, o1, seed=bytes([0x85, i]) * 16, smudge_bound=1 << 16) for i, sk in enumerate(sks)]
    opened = ctx.bfv_decrypt_combine(params, o0, np.array(shares))
    assert np.array_equal(opened[0], expected_plain(params, m, pos))


# ---- 3. the batch call against the host-array call ---------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w,n_groups,n", [(K13, 8, 1, 64), (K13, 8, 3, 64), (K13, 8, 3, 37), (P4096, 16, 1, 64), (P4096, 16, 3, 40),
                                                 (P4096, 16, 1, 600), (BIG, 16, 1, 65)],
                         ids=["K13-1x64", "K13-3x64", "K13-3x37", "P4096-1x64", "P4096-3x40", "P4096-1x600-split", "BIG-1x65-split"])
def test_batch_pack_is_the_host_array_call(ctx, keysets, params, w, n_groups, n):
    """the levels of every case have sizes on both sides of bfv_evk_wide_max, so the key set's call takes both key-switch kernels and
    the host-array call k_key_switch alone; 600 inputs at N = 4096 and 65 at N = 32768 do not fit a chunk"""
    n_ring = params[0]
    k = keysets(params, w)
    bound = ctx.bfv_evk_wide_max(params, w)
    assert 1 <= bound < n_groups * padded(n) // 2
    rng = np.random.default_rng(440 + n_ring + n)
    c0, c1 = groups_of(rng, params, n_groups, n)
    pos = rng.integers(0, n_ring, size=(n_groups, n), dtype=np.uint64)
    want = ctx.bfv_pack(params, c0, c1, k.gk0, k.gk1, pos=pos, base_bits=w)
    with ctx.bfv_cts(params, c0.reshape(-1, n_ring), c1.reshape(-1, n_ring)) as a:
        with a.pack(n, k.evk, pos=pos) as out:
            assert out.n == n_groups and same(out, want)
        held = pair(rng, params, n_groups)
        with ctx.bfv_cts(params, *held) as dst:   # a given destination, holding other data
            assert a.pack(n, k.evk, pos=pos, out=dst) is dst and same(dst, want)
        assert same(a, (c0.reshape(-1, n_ring), c1.reshape(-1, n_ring)))


# ---- 4. the fused call against the composition by hand -----------------------------------------------------------------------------

def scale_np(v, n_ring, q):
    """v nu mod Q, nu = N^-1: log2(N) exact halvings mod the odd Q, vectorised"""
    half, one = np.uint64((q >> 1) + 1), np.uint64(1)
    v = v.copy()
    for _ in range(n_ring.bit_length() - 1):
        v = (v >> one) + (v & one) * half
    return v


def by_hand(ctx, params, evk, c0, c1, pos):
    """the definition from the existing calls on batches: select, mul_monomial, add, apply_galois_evk, add; c0, c1 (n_groups, n, N)"""
    n_ring, q = params[0], params[1]
    n_groups, n = c0.shape[:2]
    width, log_n = padded(n), n_ring.bit_length() - 1
    shift = (2 * n_ring - (np.zeros((n_groups, n), dtype=np.uint64) if pos is None else pos)) % np.uint64(2 * n_ring)
    with ctx.bfv_cts(params, c0.reshape(-1, n_ring), c1.reshape(-1, n_ring)) as a:
        a.mul_monomial(shift.reshape(-1), out=a)
        moved = a.download()
    w = [np.zeros((n_groups, width, n_ring), dtype=np.uint64) for _ in range(2)]
    for comp in range(2):
        w[comp][:, :n] = scale_np(moved[comp], n_ring, q).reshape(n_groups, n, n_ring)
    cur = ctx.bfv_cts(params, w[0].reshape(-1, n_ring), w[1].reshape(-1, n_ring))
    try:
        for lv in range(1, width.bit_length()):
            h = width >> lv
            base = np.arange(n_groups)[:, None] * (2 * h) + np.arange(h)[None, :]
            with cur.select(base.reshape(-1)) as e, cur.select((base + h).reshape(-1)) as o:
                o.mul_monomial(n_ring >> lv, out=o)
                with e.add(o) as total, e.sub(o) as diff:
                    diff.apply_galois_evk((1 << lv) + 1, evk, out=diff)
                    nxt = total.add(diff)
            cur.close()
            cur = nxt
        for lv in range(width.bit_length(), log_n + 1):
            with cur.apply_galois_evk((1 << lv) + 1, evk) as switched:
                cur.add(switched, out=cur)
        return cur.download()
    finally:
        cur.close()


@pytest.mark.parametrize("params,w,n_groups,n", [(K13, 8, 1, 1024), (K13, 8, 1, 700), (P4096, 16, 2, 300), (P4096, 16, 1, 4096), (BIG, 16, 1, 3)],
                         ids=["K13-1024", "K13-700", "P4096-2x300-chunks", "P4096-4096-root-stack", "BIG-3"])
def test_fused_pack_is_the_composition_by_hand(ctx, keysets, params, w, n_groups, n):
    n_ring = params[0]
    k = keysets(params, w)
    rng = np.random.default_rng(450 + n_ring + n)
    c0, c1 = groups_of(rng, params, n_groups, n)
    pos = rng.integers(0, n_ring, size=(n_groups, n), dtype=np.uint64)
    want = by_hand(ctx, params, k.evk, c0, c1, pos)
    with ctx.bfv_cts(params, c0.reshape(-1, n_ring), c1.reshape(-1, n_ring)) as a, a.pack(n, k.evk, pos=pos) as out:
        assert same(out, want)


# ---- 5. which kernels ran ----------------------------------------------------------------------------------------------------------

def all_launches(ctx, fn):
    import zk_fhe_amd as zk
    ctx.prof_enable(True)   # resets the slots
    try:
        fn()
        return [ctx.prof_read(slot)["launches"] for slot in range(zk.PROF_BFV_PACK + 1)]
    finally:
        ctx.prof_enable(False)


def test_a_level_is_at_most_three_launches_and_no_key_is_transformed(ctx, keysets):
    import zk_fhe_amd as zk
    params, w, n = K13, 8, 64
    n_ring, log_n = params[0], params[0].bit_length() - 1
    PACK, WIDE = zk.PROF_BFV_PACK, zk.PROF_BFV_KEY_SWITCH_WIDE
    k = keysets(params, w)
    c0, c1 = groups_of(np.random.default_rng(460), params, 1, n)
    with ctx.bfv_cts(params, c0[0], c1[0]) as a, ctx.bfv_cts_zeros(params, 1) as out:
        got = all_launches(ctx, lambda: a.pack(n, k.evk, out=out))
    for slot in (zk.PROF_BFV_ELEMENTWISE, zk.PROF_BFV_GALOIS, RNS_NTT):
        assert got[slot] == 0, slot
    # k_pack_prepare, then per level one key-switch kernel and k_pack_finish; a fold for every level that goes the digit-parallel way
    pairs = [32, 16, 8, 4, 2, 1] + [1] * (log_n - 6)   # six pack levels of the 64 leaves, then the trace on the root
    bound = ctx.bfv_evk_wide_max(params, w)
    assert got[PACK] == 1 + 2 * log_n
    assert got[WIDE] == sum(1 for c in pairs if c <= bound)
    assert all(got[s] == 0 for s in range(len(got)) if s not in (PACK, WIDE))
    host = all_launches(ctx, lambda: ctx.bfv_pack(params, c0, c1, k.gk0, k.gk1, base_bits=w))
    assert host[RNS_NTT] == 1 and host[WIDE] == 0 and host[PACK] == 1 + 2 * log_n   # the one key transform; k_key_switch at every level
    assert all(host[s] == 0 for s in range(len(host)) if s not in (PACK, RNS_NTT))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def test_host_array_calls_refuse_in_order(ctx, keysets):
    import zk_fhe_amd as zk
    params, w = P8, 8
    n_ring, q = params[0], params[1]
    k = keysets(params, w)
    rng = np.random.default_rng(470)
    c0, c1 = groups_of(rng, params, 1, 3)
    over = groups_of(rng, params, 1, n_ring + 1)
    high = c0.copy()
    high[0, 1, 2] = q
    bad_pos = np.array([[0, n_ring, 1]], dtype=np.uint64)
    bad_key = k.gk1.copy()
    bad_key[1, 0, 3] = q
    even = (n_ring, q + 1, 7, 19)

    def refused(text, fn):
        with pytest.raises(zk.ZkfheError, match=text):
            fn()

    # each call breaks the rule named and the next one down the list: the earlier text wins
    refused("bfv_pack: Q must be odd", lambda: ctx.bfv_pack(even, c0, c1, k.gk0, k.gk1, base_bits=0))
    refused("bfv_pack: base_bits", lambda: ctx.bfv_pack(params, *over, k.gk0, k.gk1, base_bits=33))
    refused("bfv_pack: n = 9 is above N", lambda: ctx.bfv_pack(params, *over, k.gk0, k.gk1, pos=np.full((1, n_ring + 1), n_ring), base_bits=w))
    refused("bfv_pack: a position is not below N", lambda: ctx.bfv_pack(params, high, c1, k.gk0, k.gk1, pos=bad_pos, base_bits=w))
    refused("bfv_pack: a ciphertext coefficient", lambda: ctx.bfv_pack(params, high, c1, k.gk0, bad_key, base_bits=w))
    refused("bfv_pack: a ciphertext coefficient", lambda: ctx.bfv_pack(params, c0, high, k.gk0, k.gk1, base_bits=w))
    refused("bfv_pack: a Galois-key coefficient", lambda: ctx.bfv_pack(params, c0, c1, k.gk0, bad_key, base_bits=w))
    a = (c0[0], c1[0])
    refused("bfv_mul_monomial: k_count must be 1 or the ciphertext count", lambda: ctx.bfv_mul_monomial(params, *a, [1, 2 * n_ring]))
    refused("bfv_mul_monomial: an exponent k is not below 2N", lambda: ctx.bfv_mul_monomial(params, high[0], c1[0], [1, 2, 2 * n_ring]))
    refused("bfv_mul_monomial: an exponent k is not below 2N", lambda: ctx.bfv_mul_monomial(params, *a, 2 * n_ring))
    refused("bfv_mul_monomial: a ciphertext coefficient", lambda: ctx.bfv_mul_monomial(params, high[0], c1[0], 1))
    full = ctx.bfv_pack(params, c0, c1, k.gk0, k.gk1, pos=np.array([[n_ring - 1, 0, 1]], dtype=np.uint64), base_bits=w)   # the last position is fine
    assert full[0].shape == (1, n_ring)


def test_batch_calls_refuse_in_order_and_leave_dst_alone(ctx, keysets):
    import zk_fhe_amd as zk
    params, w = P8, 8
    n_ring, q = params[0], params[1]
    k = keysets(params, w)
    even, other = (n_ring, q + 1, 7, 19), (n_ring, q, 5, 19)
    rng = np.random.default_rng(480)
    six, d2, d3 = pair(rng, params, 6), pair(rng, params, 2), pair(rng, params, 3)
    missing = [i for i, g in enumerate(k.elements) if g != 5]   # a key set without the pack element 5
    with ctx.bfv_cts(params, *six) as a, ctx.bfv_cts(params, *d2) as dst, ctx.bfv_cts(params, *d3) as three, \
            ctx.bfv_cts(even, *six) as a_even, ctx.bfv_cts(even, *d2) as dst_even, ctx.bfv_cts(other, *d2) as alien, \
            ctx.bfv_evk(other, w, elements=k.elements, gk0=k.gk0, gk1=k.gk1) as alien_keys, \
            ctx.bfv_evk(params, w, elements=[k.elements[i] for i in missing], gk0=k.gk0[missing], gk1=k.gk1[missing]) as no_five:
        def refused(text, fn, holder=dst, held=d2):
            with pytest.raises(zk.ZkfheError, match=text):
                fn()
            assert same(holder, held), text

        bad_pos = np.array([0, 1, n_ring, 0, 0, 0], dtype=np.uint64)
        # each call breaks the rule named and the next one down the list: the earlier text wins
        refused("bfv_cts_pack: Q must be odd", lambda: a_even.pack(n_ring + 1, k.evk, out=dst_even), dst_even, d2)
        refused("bfv_cts_pack: n = 9 is above N", lambda: a.pack(n_ring + 1, k.evk, pos=np.full(2 * n_ring + 2, n_ring), out=dst))
        refused("bfv_cts_pack: a position is not below N", lambda: a.pack(3, alien_keys, pos=bad_pos, out=dst))
        refused("bfv_cts_pack: the key set and the batch have different parameters", lambda: a.pack(3, alien_keys, out=alien), alien, d2)
        refused("bfv_cts_pack: the batches have different parameters", lambda: a.pack(2, k.evk, out=alien), alien, d2)
        refused("bfv_cts_pack: a holds 6 ciphertexts and the call needs 4", lambda: a.pack(2, no_five, out=dst))
        refused("bfv_cts_pack: a holds 6 ciphertexts and the call needs 8", lambda: a.pack(4, k.evk, out=dst))
        with ctx.bfv_cts(params, *six) as src:
            refused("bfv_cts_pack: dst must not be a source", lambda: src.pack(1, no_five, out=src), src, six)
        refused("bfv_cts_pack: the key set has no key for the Galois element 5", lambda: a.pack(3, no_five, out=dst))
        refused("bfv_cts_mul_monomial: k_count must be 1 or the ciphertext count", lambda: a.mul_monomial([1, 2 * n_ring], out=dst))
        refused("bfv_cts_mul_monomial: an exponent k is not below 2N", lambda: a.mul_monomial(2 * n_ring, out=dst))
        refused("bfv_cts_mul_monomial: the batches have different parameters", lambda: three.mul_monomial(1, out=alien), alien, d2)
        refused("bfv_cts_mul_monomial: dst holds 2 ciphertexts and the call needs 3", lambda: three.mul_monomial(1, out=dst))
        with a.pack(3, k.evk) as ok, a.pack(6, k.evk) as one:   # two groups of three, one group of six
            assert ok.n == 2 and one.n == 1
        assert same(a, six) and same(three, d3)
