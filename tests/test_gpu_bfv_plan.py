"""Prepared linear-transform plans on the GPU (bfv_linear.hip): zkfhe_bfv_plan_apply bit for bit against the host-array calls
zkfhe_bfv_linear_transform and zkfhe_bfv_linear_transform_bsgs and against their Python restatements, across ciphertext chunks and
giant-step groups, reused between unrelated calls that overwrite the context's work arena, from a second context, without any
transform of a key or a diagonal on the apply path, decrypted under a single key and under a three-party collective key, and every
refusal in its order.  Run on the MI355X box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

from tests.test_bfv_bsgs_host import ref_linear_transform_bsgs
from tests.test_bfv_eval_host import Q29, Q60, Q63, relin_digits
from tests.test_bfv_galois_host import galois_element
from tests.test_bfv_linear_host import ref_linear_transform
from tests.test_gpu_bfv_bsgs import chunk_rule, grid, keys_for

pytestmark = pytest.mark.gpu
A1024 = (1024, Q29, 12289, 19)
B1024 = (1024, Q60, 12289, 19)
B4096 = (4096, Q60, 65537, 19)
B32768 = (32768, Q60, 65537, 19)
WIDE = (32768, Q63, 2013265921, 19)   # with w = 32: 159 bits already for one element, the range rule refuses
CRS = b"\xc8" * 32
PARTIES = [bytes([0x68 + i]) * 32 for i in range(3)]


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


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 2


class Case:
    """keys and diagonals of a flat transform over `flat` and of a two-level one over baby x giant, under one secret key"""

    def __init__(self, ctx, params, w, baby, giant, seed, rng):
        self.params, self.w, self.baby, self.giant, self.flat = params, w, list(baby), list(giant), list(baby) + list(giant)
        sk = ctx.bfv_fhe_keypair(params, bytes([seed]) * 32)[0]
        self.bk = keys_for(ctx, params, sk, self.baby, w, bytes([seed + 1]) * 32)
        self.hk = keys_for(ctx, params, sk, self.giant, w, bytes([seed + 2]) * 32)
        self.fk = tuple(np.concatenate([b, h]) for b, h in zip(self.bk, self.hk))
        self.fd = plaintexts(rng, params, (len(self.flat),))
        self.bd = plaintexts(rng, params, (len(self.giant), len(self.baby)))

    def flat_call(self, ctx, c0, c1):
        return ctx.bfv_linear_transform(self.params, c0, c1, self.flat, *self.fk, self.fd, base_bits=self.w)

    def bsgs_call(self, ctx, c0, c1):
        return ctx.bfv_linear_transform_bsgs(self.params, c0, c1, self.baby, *self.bk, self.giant, *self.hk, self.bd, base_bits=self.w)

    def flat_plan(self, ctx):
        return ctx.bfv_plan(self.params, self.flat, *self.fk, self.fd, base_bits=self.w)

    def bsgs_plan(self, ctx):
        return ctx.bfv_plan_bsgs(self.params, self.baby, *self.bk, self.giant, *self.hk, self.bd, base_bits=self.w)


# ---- 1. bit equality, flat and two-level -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", [(A1024, 4), (B4096, 16)])
def test_apply_is_the_host_array_call(ctx, params, w):
    import zk_fhe_amd as zk
    n = params[0]
    rng = np.random.default_rng(41)
    case = Case(ctx, params, w, *grid(n), 0xb0, rng)
    c0, c1 = residues(rng, params, 3), residues(rng, params, 3)
    with case.flat_plan(ctx) as plan:
        assert isinstance(plan, zk.BfvLinearPlan)
        got = plan.apply(c0, c1)
        assert got[0].shape == got[1].shape == (3, n)
        assert same(got, case.flat_call(ctx, c0, c1))
        r = ref_linear_transform(params, c0[1], c1[1], case.flat, *case.fk, w, case.fd)
        assert np.array_equal(got[0][1], r[0]) and np.array_equal(got[1][1], r[1])
    with case.bsgs_plan(ctx) as plan:
        got = plan.apply(c0, c1)
        assert same(got, case.bsgs_call(ctx, c0, c1))
        r = ref_linear_transform_bsgs(params, c0[2], c1[2], case.baby, *case.bk, case.giant, *case.hk, w, case.bd)
        assert np.array_equal(got[0][2], r[0]) and np.array_equal(got[1][2], r[1])
    assert plan.h is None
    with pytest.raises(zk.ZkfheError, match="closed"):
        plan.apply(c0, c1)


# ---- 2. across chunks and groups -------------------------------------------------------------------------------------------------

def test_flat_across_a_ciphertext_chunk(ctx):
    """13 ciphertexts at N = 32768, w = 16: l + 1 = 5 hoisted rows per ciphertext against chunk_polys(N) = 64 polynomials, so the flat
    loop takes 12 ciphertexts and then 1"""
    params, w, count = B32768, 16, 13
    n = params[0]
    assert relin_digits(params[1], w) + 1 == 5 and min(count, max(8, (1 << 21) // n) // 5) == 12 < count
    rng = np.random.default_rng(42)
    case = Case(ctx, params, w, [galois_element(n, 3), 1], [2 * n - 1], 0xb3, rng)
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    with case.flat_plan(ctx) as plan:
        assert same(plan.apply(c0, c1), case.flat_call(ctx, c0, c1))


def test_bsgs_across_a_ciphertext_chunk(ctx):
    """58 ciphertexts at N = 1024, w = 4 with the 3 x 3 grid: chunks of 56 and 2, one group of giant steps"""
    params, w, count = A1024, 4, 58
    assert chunk_rule(params, w, count, 3, 3) == (56, 3)
    rng = np.random.default_rng(43)
    case = Case(ctx, params, w, *grid(params[0]), 0xb6, rng)
    c0, c1 = residues(rng, params, count), residues(rng, params, count)
    with case.bsgs_plan(ctx) as plan:
        assert same(plan.apply(c0, c1), case.bsgs_call(ctx, c0, c1))


def test_bsgs_across_a_giant_group(ctx):
    """one ciphertext at N = 1024, w = 1 (30 hoisted rows) with 2 baby and 70 giant steps: groups of 68 and 2 giant steps"""
    params, w, n_giant = A1024, 1, 70
    n = params[0]
    assert chunk_rule(params, w, 1, 2, n_giant) == (1, 68)
    rng = np.random.default_rng(44)
    cycle = [galois_element(n, 5), 2 * n - 1, 1, galois_element(n, 9, True)]
    case = Case(ctx, params, w, [galois_element(n, 1), 1], [cycle[i % 4] for i in range(n_giant)], 0xb9, rng)
    c0, c1 = residues(rng, params, 1), residues(rng, params, 1)
    with case.bsgs_plan(ctx) as plan:
        assert plan.info()["key_slots"] == 1 + 53   # every fourth giant element is g = 1
        assert same(plan.apply(c0, c1), case.bsgs_call(ctx, c0, c1))


# ---- 3. reuse, between calls that overwrite the work arena -----------------------------------------------------------------------

@pytest.mark.parametrize("two_level", [False, True])
def test_one_plan_many_applies(ctx, two_level):
    params, w = B1024, 8
    rng = np.random.default_rng(45)
    case = Case(ctx, params, w, *grid(params[0]), 0xbc, rng)
    sk = ctx.bfv_fhe_keypair(params, b"\xbf" * 32)[0]
    rlk0, rlk1 = ctx.bfv_relin_keygen(params, sk, seed=b"\xc0" * 32, base_bits=w)
    plan = case.bsgs_plan(ctx) if two_level else case.flat_plan(ctx)
    host = case.bsgs_call if two_level else case.flat_call
    try:
        for count in (1, 5, 2):
            c0, c1 = residues(rng, params, count), residues(rng, params, count)
            assert same(plan.apply(c0, c1), host(ctx, c0, c1)), count
            # an unrelated call on the same context: 40 products fill the front of the work arena with other data
            a = [residues(rng, params, 40) for _ in range(4)]
            ctx.bfv_mul(params, *a, rlk0, rlk1, base_bits=w)
            ctx.bfv_sum(params, a[0], a[1])
            assert same(plan.apply(c0, c1), host(ctx, c0, c1)), count
    finally:
        plan.close()
    plan.close()   # a second close is nothing


# ---- 4. no preparation on the apply path -----------------------------------------------------------------------------------------

def launches(ctx, fn):
    import zk_fhe_amd as zk
    ctx.prof_enable(True)   # resets the slots
    try:
        out = fn()
        slots = {name: ctx.prof_read(getattr(zk, "PROF_" + name))["launches"]
                 for name in ("RNS_NTT", "BFV_HOIST", "BFV_LINEAR", "BFV_BSGS_INNER", "BFV_BSGS_GIANT", "BFV_EVAL_EPILOGUE")}
    finally:
        ctx.prof_enable(False)
    return out, slots


@pytest.mark.parametrize("identity", [False, True])
def test_apply_transforms_no_key_and_no_diagonal(ctx, identity):
    """the host-array call transforms the keys in one launch (when an element has g != 1) and the diagonals in one: RNS_NTT counts
    2 (or 1) launches more than apply, and every other slot the same"""
    params, w = B1024, 8
    n = params[0]
    rng = np.random.default_rng(46)
    case = Case(ctx, params, w, [1, 1] if identity else grid(n)[0], [1] if identity else grid(n)[1], 0xc1, rng)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    for host, make in ((case.flat_call, case.flat_plan), (case.bsgs_call, case.bsgs_plan)):
        want, called = launches(ctx, lambda: host(ctx, c0, c1))
        with make(ctx) as plan:
            assert plan.info()["key_slots"] == (0 if identity else sum(g != 1 for g in case.flat))
            got, applied = launches(ctx, lambda: plan.apply(c0, c1))
        assert same(got, want)
        assert called.pop("RNS_NTT") - applied.pop("RNS_NTT") == (1 if identity else 2)
        assert called == applied and called["BFV_HOIST"] >= 1 and called["BFV_EVAL_EPILOGUE"] >= 1


# ---- 5. a second context ---------------------------------------------------------------------------------------------------------

def test_a_second_context_applies_the_plan(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 8
    rng = np.random.default_rng(47)
    case = Case(ctx, params, w, *grid(params[0]), 0xc4, rng)
    c0, c1 = residues(rng, params, 3), residues(rng, params, 3)
    other = zk.Context(0)
    try:
        for make, host in ((case.flat_plan, case.flat_call), (case.bsgs_plan, case.bsgs_call)):
            with make(ctx) as plan:
                want = host(ctx, c0, c1)
                assert same(plan.apply(c0, c1, ctx=other), want)
                assert same(plan.apply(c0, c1), want)
                other.sync()
    finally:
        other.close()


# ---- 6. decryption ---------------------------------------------------------------------------------------------------------------

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
    return (m @ v.astype(np.int64) % params[2]).astype(np.uint64)   # entries below 2^14, N = 2^10: below 2^38


def test_banded_matrix_decrypts_through_a_plan(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 8
    n, q, t = params[:3]
    l = relin_digits(q, w)
    rng = np.random.default_rng(48)
    m = banded(rng, params, (0, 1, 2, 5), (0, 3))
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, m, 2)
    assert len(g_baby) == 2 and len(g_giant) == 5
    diag = ctx.bfv_encode_slots(params, d.reshape(-1, n)).reshape(d.shape)
    v = rng.integers(0, t, size=(2, n), dtype=np.uint64)
    want = np.array([matvec(params, m, x) for x in v])

    # under a single key
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\xc7" * 32)
    bk0, bk1 = keys_for(ctx, params, sk, g_baby, w, b"\xc9" * 32)
    hk0, hk1 = keys_for(ctx, params, sk, g_giant, w, b"\xca" * 32)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\xcb" * 32)
    with ctx.bfv_plan_bsgs(params, g_baby, bk0, bk1, g_giant, hk0, hk1, diag, base_bits=w) as plan:
        o0, o1 = plan.apply(ct["c0"], ct["c1"])
    assert int(ctx.bfv_noise(params, sk, o0, o1).max()) < (q // t) // 2
    assert np.array_equal(ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, o0, o1)), want)

    # under the collective key of three parties
    keys = [ctx.bfv_keygen_share(params, CRS, ps) for ps in PARTIES]
    sks = [k[0] for k in keys]
    pk0, pk1 = ctx.bfv_share_aggregate(params, np.array([k[1] for k in keys])), keys[0][2]

    def joint(elements):
        k0, k1 = np.zeros((len(elements), l, n), dtype=np.uint64), np.zeros((len(elements), l, n), dtype=np.uint64)
        for i, g in enumerate(elements):
            if g == 1:
                continue   # never read
            shares = [ctx.bfv_galois_share(params, s, CRS, ps, g, base_bits=w) for s, ps in zip(sks, PARTIES)]
            k0[i], k1[i] = ctx.bfv_share_aggregate(params, np.array([s[0] for s in shares])), shares[0][1]
        return k0, k1

    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, v), b"\xcc" * 32)
    with ctx.bfv_plan_bsgs(params, g_baby, *joint(g_baby), g_giant, *joint(g_giant), diag, base_bits=w) as plan:
        o0, o1 = plan.apply(ct["c0"], ct["c1"])
    shares = [ctx.bfv_decrypt_share(params, s, o1, seed=bytes([0x7a, i]) * 16, smudge_bound=1 << 20) for i, s in enumerate(sks)]
    assert np.array_equal(ctx.bfv_decode_slots(params, ctx.bfv_decrypt_combine(params, o0, np.array(shares))), want)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------

RANGE = "narrow base_bits, or split the element list"
KEY = "Galois-key coefficient is not below Q"
DIAG = "a diagonal coefficient is outside"
ODD = "every Galois element g must be odd and below 2N"
BITS = r"base_bits must be in \[1, 32\]"


def test_creation_refusals_in_order(ctx):
    """every refusal of the host-array calls that does not concern a ciphertext, under the plan's prefix; an input that breaks two
    rules reports the earlier one"""
    import zk_fhe_amd as zk
    params = B1024
    n, q, t = params[:3]
    l = relin_digits(q, 16)
    keys, bad_key = np.zeros((2, l, n), dtype=np.uint64), np.zeros((2, l, n), dtype=np.uint64)
    bad_key[1, 1, 2] = q
    d1, d2 = np.zeros((2, n), dtype=np.uint64), np.zeros((2, 2, n), dtype=np.uint64)

    def flat(g=(5, 3), k0=keys, k1=keys, d=d1, w=16, prm=params):
        return ctx.bfv_plan(prm, list(g), k0, k1, d, base_bits=w)

    def bsgs(gb=(5, 3), bk0=keys, bk1=keys, gg=(25, 3), hk0=keys, hk1=keys, d=d2, w=16, prm=params):
        return ctx.bfv_plan_bsgs(prm, list(gb), bk0, bk1, list(gg), hk0, hk1, d, base_bits=w)

    def refused(fn, prefix, text, **kw):
        with pytest.raises(zk.ZkfheError, match=(prefix + ": " if prefix else "") + ".*" + text):
            fn(**kw)

    F, S = "bfv_plan_create", "bfv_plan_create_bsgs"
    flat().close(), bsgs().close()   # the arguments, whole
    bad_d1, bad_d2 = d1.copy(), d2.copy()
    bad_d1[1, 7] = bad_d2[1, 0, 7] = t // 2 + 1
    # each rule alone
    for w in (0, 33):
        refused(flat, F, BITS, w=w), refused(bsgs, S, BITS, w=w)
    for g in (0, 4, 2 * n, 2 * n + 1):
        refused(flat, F, ODD, g=(5, g)), refused(bsgs, S, ODD, gb=(5, g)), refused(bsgs, S, ODD, gg=(g, 5))
    for name in ("k0", "k1"):
        refused(flat, F, KEY, **{name: bad_key})
    for name in ("bk0", "bk1", "hk0", "hk1"):
        refused(bsgs, S, KEY, **{name: bad_key})
    for value in (t // 2 + 1, q - t // 2 - 1, q):
        x1, x2 = d1.copy(), d2.copy()
        x1[1, 7] = x2[1, 0, 7] = value
        refused(flat, F, DIAG, d=x1), refused(bsgs, S, DIAG, d=x2)
    # bad parameters (the text of every BFV call), and before base_bits
    k1000 = np.zeros((2, l, 1000), np.uint64)
    p1000 = (1000, q, t, 19)
    for w in (16, 0):
        refused(flat, "", "bfv params", k0=k1000, k1=k1000, d=np.zeros((2, 1000), np.uint64), prm=p1000, w=w)
        refused(bsgs, "", "bfv params", bk0=k1000, bk1=k1000, hk0=k1000, hk1=k1000, d=np.zeros((2, 2, 1000), np.uint64), prm=p1000, w=w)
    # a bad g before a bad key before a bad diagonal
    refused(flat, F, ODD, g=(5, 4), k0=bad_key, d=bad_d1), refused(bsgs, S, ODD, gg=(25, 4), hk1=bad_key, d=bad_d2)
    refused(flat, F, KEY, k1=bad_key, d=bad_d1), refused(bsgs, S, KEY, bk0=bad_key, d=bad_d2)

    # the range rule: after a bad g, before the passes over the keys and the diagonals, and before any device work
    lw = relin_digits(Q63, 32)
    wide_keys = np.full((1, lw, WIDE[0]), Q63, dtype=np.uint64)   # a bad key and a bad diagonal, were they looked at
    wide_d = np.full((1, 1, WIDE[0]), Q63, dtype=np.uint64)
    ctx.prof_enable(True)
    try:
        refused(flat, F, RANGE, g=(5,), k0=wide_keys, k1=wide_keys, d=wide_d[0], w=32, prm=WIDE)
        refused(bsgs, S, RANGE, gb=(5,), bk0=wide_keys, bk1=wide_keys, gg=(25,), hk0=wide_keys, hk1=wide_keys, d=wide_d, w=32, prm=WIDE)
        for slot in range(5, 20):
            assert ctx.prof_read(slot)["launches"] == 0, slot
    finally:
        ctx.prof_enable(False)
    refused(flat, F, ODD, g=(4,), k0=wide_keys, k1=wide_keys, d=wide_d[0], w=32, prm=WIDE)
    refused(bsgs, S, ODD, gb=(5,), bk0=wide_keys, bk1=wide_keys, gg=(2 * WIDE[0],), hk0=wide_keys, hk1=wide_keys, d=wide_d, w=32, prm=WIDE)

    # at the C boundary: NULL pointers, zero counts, counts of 2^20, and *out after a failure
    u64p, vp = ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    lib, prm, bad_prm = ctx.lib, zk.BfvParamsC(*params), zk.BfvParamsC(*p1000)
    g = np.array([5, 3], dtype=np.uint64)
    gp, kp, dp = g.ctypes.data_as(u64p), keys.ctypes.data_as(u64p), d2.ctypes.data_as(u64p)
    for name, fn, good, counts, bits in (
            (F, lib.zkfhe_bfv_plan_create, [2, gp, kp, kp, 16, dp], (0,), 4),
            (S, lib.zkfhe_bfv_plan_create_bsgs, [2, gp, kp, kp, 2, gp, kp, kp, 16, dp], (0, 4), 8)):

        def create(args, p=prm):
            h = vp(0xdead0)   # whatever the caller left there
            rc = fn(ctx.h, ctypes.byref(p), *args, ctypes.byref(h))
            return rc, h, lib.zkfhe_last_error(ctx.h).decode()

        for pos in range(len(good)):
            if pos == bits:
                continue
            broken = list(good)
            broken[pos] = 0 if pos in counts else None
            rc, h, text = create(broken, bad_prm)   # and before the parameters
            assert rc != 0 and h.value is None and text.startswith(name + ": a NULL argument or a zero count"), (name, pos, text)
        broken = list(good)
        broken[bits] = 0
        rc, h, text = create(broken, bad_prm)   # bad parameters before base_bits
        assert rc != 0 and h.value is None and text.startswith("bfv params"), (name, text)
        assert fn(ctx.h, ctypes.byref(prm), *good, None) != 0   # out itself
        assert lib.zkfhe_last_error(ctx.h).decode().startswith(name + ": a NULL argument")
        for pos in counts:   # the count is refused before the list is read, after base_bits
            broken = list(good)
            broken[pos] = 1 << 20
            rc, h, text = create(broken)
            assert rc != 0 and h.value is None and text == name + ": more than 2^20 Galois elements", (name, pos, text)
            broken[bits] = 0
            rc, h, text = create(broken)
            assert rc != 0 and h.value is None and text == name + ": base_bits must be in [1, 32]", (name, pos, text)
        rc, h, text = create(good)
        assert rc == 0 and h.value
        assert lib.zkfhe_bfv_plan_destroy(ctx.h, h) == 0


def test_apply_refusals_write_nothing(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 16
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    keys = np.zeros((2, l, n), dtype=np.uint64)
    z = np.zeros((2, n), dtype=np.uint64)
    big = z.copy()
    big[1, 3] = q
    u64p = ctypes.POINTER(ctypes.c_uint64)
    fn = ctx.lib.zkfhe_bfv_plan_apply
    plans = [ctx.bfv_plan(params, [5, 3], keys, keys, z, base_bits=w),
             ctx.bfv_plan_bsgs(params, [5, 3], keys, keys, [25, 3], keys, keys, np.zeros((2, 2, n), np.uint64), base_bits=w)]
    try:
        for plan in plans:
            for kw in ((big, z), (z, big)):
                with pytest.raises(zk.ZkfheError, match="bfv_plan_apply: a ciphertext coefficient is not below Q"):
                    plan.apply(*kw)
            mark = np.uint64(0x5a5a5a5a5a5a5a5a)
            out = [np.full((2, n), mark), np.full((2, n), mark)]
            zp, bp, o0, o1 = (a.ctypes.data_as(u64p) for a in (z, big, *out))
            good = [ctx.h, plan.h, 2, zp, zp, o0, o1]
            for pos in range(1, len(good)):
                broken = list(good)
                broken[pos] = 0 if pos == 2 else None
                assert fn(*broken) != 0, pos
                assert ctx.lib.zkfhe_last_error(ctx.h).decode().startswith("bfv_plan_apply: a NULL argument or a zero count"), pos
            assert fn(ctx.h, plan.h, 2, zp, bp, o0, o1) != 0
            assert ctx.lib.zkfhe_last_error(ctx.h).decode().startswith("bfv_plan_apply: a ciphertext coefficient is not below Q")
            assert (out[0] == mark).all() and (out[1] == mark).all()   # nothing was written
            assert fn(*good) == 0 and not out[0].any() and not out[1].any()   # the same arguments, whole
        import torch
        if torch.cuda.device_count() > 1:   # a context of another device, where the box has one
            other = zk.Context(1)
            try:
                with pytest.raises(zk.ZkfheError, match="bfv_plan_apply: the plan lives on device 0"):
                    plans[0].apply(z, z, ctx=other)
            finally:
                other.close()
    finally:
        for plan in plans:
            plan.close()


def test_info_and_the_key_rows_of_identity_elements(ctx):
    import zk_fhe_amd as zk
    params, w = B1024, 8
    n, q = params[0], params[1]
    rng = np.random.default_rng(49)
    g_baby, g_giant = [1, galois_element(n, 2), 1], [galois_element(n, 4), 1]
    case = Case(ctx, params, w, g_baby, g_giant, 0xcd, rng)
    c0, c1 = residues(rng, params, 2), residues(rng, params, 2)
    want_flat, want_bsgs = case.flat_call(ctx, c0, c1), case.bsgs_call(ctx, c0, c1)
    for k in (0, 2):   # the rows of g = 1: values no key may hold
        case.bk[0][k], case.bk[1][k] = np.uint64(q), np.uint64(2 ** 64 - 1)
    case.hk[0][1], case.hk[1][1] = np.uint64(2 ** 64 - 1), np.uint64(q)
    case.fk = tuple(np.concatenate([b, h]) for b, h in zip(case.bk, case.hk))
    with case.flat_plan(ctx) as plan:
        info = plan.info()
        assert info == {"params": params, "base_bits": w, "n_elems": 5, "n_giant": 0, "key_slots": 2,
                        "device_bytes": zk.bfv_plan_bytes(params, w, 5, 2, 5)}
        assert same(plan.apply(c0, c1), want_flat)
    with case.bsgs_plan(ctx) as plan:
        info = plan.info()
        assert info == {"params": params, "base_bits": w, "n_elems": 3, "n_giant": 2, "key_slots": 2,
                        "device_bytes": zk.bfv_plan_bytes(params, w, 3 + 2, 2, 3 * 2)}
        assert info["device_bytes"] == 4 * (2 * 5 + 2 * 2 * relin_digits(q, w) * n * 5 + 6 * n * 5)
        assert same(plan.apply(c0, c1), want_bsgs)
    # all-identity lists hold no key at all
    with ctx.bfv_plan_bsgs(params, [1], case.bk[0][:1], case.bk[1][:1], [1], case.hk[0][1:], case.hk[1][1:], case.bd[:1, :1], base_bits=w) as plan:
        assert plan.info()["key_slots"] == 0 and plan.info()["device_bytes"] == 4 * (4 + n * 5)
        p0, p1 = ctx.bfv_mul_plain(params, c0, c1, case.bd[0, 0])
        assert same(plan.apply(c0, c1), (p0, p1))
