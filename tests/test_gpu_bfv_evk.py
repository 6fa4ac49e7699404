"""Resident evaluation keys on the GPU (bfv_evk.hip) and the calls on batches that take them (bfv_resident.hip): every call bit for
bit against the host-array call on the downloaded sources, at one and three ciphertexts (where the digit-parallel key switch runs
when l >= 2), at one count just above Context.bfv_evk_wide_max (where k_key_switch runs), with w = 32 (l = 1: never digit-parallel),
across a ciphertext chunk at N = 32768, and with the destination aliasing a source where that is allowed; which kernels ran, from
the profiling slots; the inner products against mul_evk, bfv_sum and bfv_mul_plain; a chain from the ballot box to the slot sum that
never visits the host; a second context; the refusals.  The reference of every value is a host-array call.
Run on the MI355X box: pytest -m gpu."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60
from tests.test_gpu_bfv_ballot import make_ballots
from tests.test_gpu_bfv_bsgs import grid
from tests.test_gpu_bfv_plan import Case, plaintexts
from tests.test_gpu_bfv_resident import check_call, pair, same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P8 = (8, Q29, 7, 19)
K13 = (1024, Q29, 7, 19)
P4096 = (4096, Q60, 65537, 19)
BIG = (32768, Q60, 65537, 19)   # chunk_polys(N) = 64
CROSS = 65
CASES = [(P8, 8), (P8, 32), (K13, 8), (P4096, 8), (P4096, 16)]   # l = 4, 1, 4, 8, 4
RNS_NTT = 6   # the slot of k_rns_ntt: the key transform of a host-array call, and the transforms of the operands


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


class Keys:
    """one secret key's relinearization key and the Galois keys of bfv_slot_sum_elements (5 and 2N - 1 among them), as host arrays
    and as a key set; fixed seeds"""

    def __init__(self, ctx, params, w, relin=True):
        import zk_fhe_amd as zk
        self.params, self.w = params, w
        self.sk = ctx.bfv_fhe_keypair(params, b"\x71" * 32)[0]
        self.rlk = ctx.bfv_relin_keygen(params, self.sk, b"\x72" * 32, base_bits=w) if relin else None
        self.elements = [int(g) for g in zk.bfv_slot_sum_elements(params)]
        keys = [ctx.bfv_galois_keygen(params, self.sk, g, seed=b"\x73" * 32, base_bits=w) for g in self.elements]
        self.gk0, self.gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
        self.evk = ctx.bfv_evk(params, w, self.rlk, self.elements, self.gk0, self.gk1)

    def galois(self, g):
        i = self.elements.index(g)
        return self.gk0[i], self.gk1[i]


@pytest.fixture(scope="module")
def keysets(ctx):
    made = {}

    def get(params, w):
        if (params, w) not in made:
            made[(params, w)] = Keys(ctx, params, w)
        return made[(params, w)]

    yield get
    for k in made.values():
        k.evk.close()


def counts(ctx, params, w):
    """one and three ciphertexts, and the first count past the digit-parallel path"""
    return sorted({1, 3, ctx.bfv_evk_wide_max(params, w) + 1})


@pytest.fixture(scope="module")
def big(ctx):
    rng = np.random.default_rng(165)
    a, b = pair(rng, BIG, CROSS), pair(rng, BIG, CROSS)
    for x in a + b:
        x.setflags(write=False)
    return a, b


# ---- 1. the key set --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", CASES)
def test_info_and_size(ctx, keysets, params, w):
    import zk_fhe_amd as zk
    k = keysets(params, w)
    l = zk.bfv_relin_digits(params, w)
    info = k.evk.info()
    assert isinstance(k.evk, zk.BfvEvalKeys) and k.evk.params == params
    assert info == {"params": params, "base_bits": w, "has_relin": True, "elements": k.elements,
                    "device_bytes": (1 + len(k.elements)) * 2 * l * 5 * params[0] * 4}
    assert info["device_bytes"] == zk.bfv_evk_bytes(params, w, True, len(k.elements))
    bound = ctx.bfv_evk_wide_max(params, w)
    assert (bound == 0) == (l == 1) and bound * l <= max(8, (1 << 21) // params[0])


def test_halves_alone_and_closing(ctx):
    import zk_fhe_amd as zk
    k = Keys(ctx, P8, 8)
    k.evk.close()
    with pytest.raises(zk.ZkfheError, match="closed"):
        k.evk.info()
    with ctx.bfv_evk(P8, 8, rlk=k.rlk) as only_relin:
        assert only_relin.info()["elements"] == [] and only_relin.info()["has_relin"]
    with ctx.bfv_evk(P8, 8, elements=[5], gk0=k.gk0[:1], gk1=k.gk1[:1]) as only_galois:
        assert only_galois.info()["elements"] == [5] and not only_galois.info()["has_relin"]
        assert only_galois.info()["device_bytes"] == zk.bfv_evk_bytes(P8, 8, False, 1)


# ---- 2. every call against the host-array call -----------------------------------------------------------------------------------

@pytest.mark.parametrize("params,w", CASES)
def test_mul_evk(ctx, keysets, params, w):
    k = keysets(params, w)
    for count in counts(ctx, params, w):
        rng = np.random.default_rng(200 + count)
        a, b = pair(rng, params, count), pair(rng, params, count)
        host = lambda a0, a1, b0, b1: ctx.bfv_mul(params, a0, a1, b0, b1, *k.rlk, base_bits=w)  # noqa: E731
        check_call(ctx, params, [a, b], host, lambda x, y, out: x.mul_evk(y, k.evk, out=out))


@pytest.mark.parametrize("params,w", CASES)
def test_apply_galois_evk(ctx, keysets, params, w):
    k = keysets(params, w)
    for count in counts(ctx, params, w):
        a = pair(np.random.default_rng(210 + count), params, count)
        for g in (5, 2 * params[0] - 1):
            gk0, gk1 = k.galois(g)
            host = lambda c0, c1: ctx.bfv_apply_galois(params, c0, c1, g, gk0, gk1, base_bits=w)  # noqa: E731
            check_call(ctx, params, [a], host, lambda x, out: x.apply_galois_evk(g, k.evk, out=out))


@pytest.mark.parametrize("params,w", CASES)
def test_slot_sum(ctx, keysets, params, w):
    k = keysets(params, w)
    for count in counts(ctx, params, w):
        a = pair(np.random.default_rng(220 + count), params, count)
        host = lambda c0, c1: ctx.bfv_slot_sum(params, c0, c1, k.gk0, k.gk1, base_bits=w)  # noqa: E731
        check_call(ctx, params, [a], host, lambda x, out: x.slot_sum(k.evk, out=out))


def dot_operands(rng, params, n_groups, n_terms):
    n, q = params[0], params[1]
    return [rng.integers(0, q, size=(n_groups, n_terms, n), dtype=np.uint64) for _ in range(4)]


@pytest.mark.parametrize("params,w", CASES)
def test_dot(ctx, keysets, params, w):
    k = keysets(params, w)
    n = params[0]
    for n_groups in counts(ctx, params, w):
        for n_terms in (1, 5):
            a0, a1, b0, b1 = dot_operands(np.random.default_rng(230 + n_groups + n_terms), params, n_groups, n_terms)
            with ctx.bfv_cts(params, a0.reshape(-1, n), a1.reshape(-1, n)) as x:
                # one b per group
                want = ctx.bfv_dot(params, a0, a1, b0, b1, *k.rlk, base_bits=w)
                with ctx.bfv_cts(params, b0.reshape(-1, n), b1.reshape(-1, n)) as y, x.dot(y, n_terms, k.evk) as out:
                    assert out.info()["n"] == n_groups and same(out, want)
                    if n_terms == 1:
                        with x.mul_evk(y, k.evk) as prod:
                            assert same(prod, want)
                # one b shared by every group
                want = ctx.bfv_dot(params, a0, a1, b0[0], b1[0], *k.rlk, base_bits=w)
                with ctx.bfv_cts(params, b0[0], b1[0]) as y, ctx.bfv_cts_zeros(params, n_groups) as dst:
                    assert x.dot(y, n_terms, k.evk, out=dst) is dst and same(dst, want)
                assert same(x, (a0.reshape(-1, n), a1.reshape(-1, n)))


@pytest.mark.parametrize("params,w", CASES)
def test_dot_plain(ctx, params, w):
    n = params[0]
    for n_groups in (1, 3):
        for n_terms in (1, 5):
            rng = np.random.default_rng(240 + n_groups + n_terms)
            a0, a1, _, _ = dot_operands(rng, params, n_groups, n_terms)
            m = plaintexts(rng, params, (n_groups, n_terms))
            with ctx.bfv_cts(params, a0.reshape(-1, n), a1.reshape(-1, n)) as x:
                for weights in (m, m[0]):   # one weight vector per group, one for every group
                    want = ctx.bfv_dot_plain(params, a0, a1, weights)
                    with x.dot_plain(weights, n_terms) as out:
                        assert out.info()["n"] == n_groups and same(out, want)
                    for g in range(n_groups):   # the definition: the sum of the products
                        mg = weights[g] if weights.ndim == 3 else weights
                        p0, p1 = ctx.bfv_mul_plain(params, a0[g], a1[g], mg)
                        s0, s1 = ctx.bfv_sum(params, p0, p1)
                        assert np.array_equal(s0, want[0][g]) and np.array_equal(s1, want[1][g])


def test_mul_evk_across_a_chunk(ctx, big):
    a, b = big
    w = 32
    sk = ctx.bfv_fhe_keypair(BIG, b"\x74" * 32)[0]
    rlk = ctx.bfv_relin_keygen(BIG, sk, b"\x75" * 32, base_bits=w)
    with ctx.bfv_evk(BIG, w, rlk=rlk) as evk:
        host = lambda a0, a1, b0, b1: ctx.bfv_mul(BIG, a0, a1, b0, b1, *rlk, base_bits=w)  # noqa: E731
        want = host(*a, *b)
        with ctx.bfv_cts(BIG, *a) as x, ctx.bfv_cts(BIG, *b) as y:
            assert x.mul_evk(y, evk, out=x) is x and same(x, want) and same(y, b)   # the destination is a source


def test_apply_galois_evk_across_a_chunk(ctx, big):
    a, _ = big
    w, g = 16, 5
    sk = ctx.bfv_fhe_keypair(BIG, b"\x76" * 32)[0]
    gk0, gk1 = ctx.bfv_galois_keygen(BIG, sk, g, seed=b"\x77" * 32, base_bits=w)
    with ctx.bfv_evk(BIG, w, elements=[g], gk0=gk0[None], gk1=gk1[None]) as evk:
        want = ctx.bfv_apply_galois(BIG, *a, g, gk0, gk1, base_bits=w)
        with ctx.bfv_cts(BIG, *a) as x:
            assert x.apply_galois_evk(g, evk, out=x) is x and same(x, want)


def test_slot_sum_at_the_largest_ring_uses_all_fifteen_keys(ctx):
    w, count = 16, 2
    k = Keys(ctx, BIG, w, relin=False)
    try:
        assert len(k.elements) == 15 and 1 <= count <= ctx.bfv_evk_wide_max(BIG, w)   # 128 KiB of LDS per workgroup, digit-parallel
        a = pair(np.random.default_rng(250), BIG, count)
        want = ctx.bfv_slot_sum(BIG, *a, k.gk0, k.gk1, base_bits=w)
        with ctx.bfv_cts(BIG, *a) as x, x.slot_sum(k.evk) as out:
            assert same(out, want) and same(x, a)
    finally:
        k.evk.close()


def test_slot_sum_across_a_chunk(ctx, big):
    """65 ciphertexts in place: the batch call with the key set and the host-array call both cross a chunk, each with all fifteen
    keys, in one loop; w = 32 gives l = 2, the smallest keys"""
    a, _ = big
    w = 32
    k = Keys(ctx, BIG, w, relin=False)
    try:
        want = ctx.bfv_slot_sum(BIG, *a, k.gk0, k.gk1, base_bits=w)
        with ctx.bfv_cts(BIG, *a) as x:
            assert x.slot_sum(k.evk, out=x) is x and same(x, want)   # the destination is the source
    finally:
        k.evk.close()


# ---- 3. which kernels ran --------------------------------------------------------------------------------------------------------

def all_launches(ctx, fn):
    import zk_fhe_amd as zk
    ctx.prof_enable(True)   # resets the slots
    try:
        fn()
        return [ctx.prof_read(slot)["launches"] for slot in range(zk.PROF_BFV_KEY_SWITCH_WIDE + 1)]
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("params,w", [(K13, 8), (P4096, 16)])
def test_the_digit_parallel_key_switch_runs_up_to_the_bound_and_no_key_is_transformed(ctx, keysets, params, w):
    import zk_fhe_amd as zk
    WIDE, GALOIS, RELIN = zk.PROF_BFV_KEY_SWITCH_WIDE, zk.PROF_BFV_GALOIS, zk.PROF_BFV_RELIN
    k = keysets(params, w)
    bound = ctx.bfv_evk_wide_max(params, w)
    steps = len(k.elements)
    assert bound >= 3
    for count in (1, bound, bound + 1):
        wide = count <= bound
        rng = np.random.default_rng(260 + count)
        a, b = pair(rng, params, count), pair(rng, params, count)
        with ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y, ctx.bfv_cts_zeros(params, count) as out:
            calls = [
                (1, RELIN, lambda: ctx.bfv_mul(params, *a, *b, *k.rlk, base_bits=w), lambda: x.mul_evk(y, k.evk, out=out)),
                (1, GALOIS, lambda: ctx.bfv_apply_galois(params, *a, 5, *k.galois(5), base_bits=w), lambda: x.apply_galois_evk(5, k.evk, out=out)),
                (steps, GALOIS, lambda: ctx.bfv_slot_sum(params, *a, k.gk0, k.gk1, base_bits=w), lambda: x.slot_sum(k.evk, out=out)),
            ]
            for switches, slot, host, call in calls:
                want, got = all_launches(ctx, host), all_launches(ctx, call)
                assert want[WIDE] == 0 and got[RNS_NTT] == want[RNS_NTT] - 1   # the one launch that transforms the key, or the keys
                assert got[WIDE] == (2 * switches if wide else 0)
                assert got[slot] == want[slot] - (switches if wide else 0)     # k_key_switch, where the two kernels replace it
                rest = [s for s in range(len(got)) if s not in (RNS_NTT, WIDE, slot)]
                assert [got[s] for s in rest] == [want[s] for s in rest]
        # the inner product: one key switch per call
        a0, a1, b0, b1 = dot_operands(rng, params, count, 2)
        n = params[0]
        with ctx.bfv_cts(params, a0.reshape(-1, n), a1.reshape(-1, n)) as x, ctx.bfv_cts(params, b0.reshape(-1, n), b1.reshape(-1, n)) as y, \
                ctx.bfv_cts_zeros(params, count) as out:
            want = all_launches(ctx, lambda: ctx.bfv_dot(params, a0, a1, b0, b1, *k.rlk, base_bits=w))
            got = all_launches(ctx, lambda: x.dot(y, 2, k.evk, out=out))
            assert got[RNS_NTT] == want[RNS_NTT] - 1 and got[WIDE] == (2 if wide else 0) and got[RELIN] == (0 if wide else 1)
            rest = [s for s in range(len(got)) if s not in (RNS_NTT, WIDE, RELIN)]
            assert [got[s] for s in rest] == [want[s] for s in rest]


def test_one_digit_never_takes_the_digit_parallel_path(ctx, keysets):
    import zk_fhe_amd as zk
    k = keysets(P8, 32)
    assert ctx.bfv_evk_wide_max(P8, 32) == 0
    a = pair(np.random.default_rng(270), P8, 1)
    with ctx.bfv_cts(P8, *a) as x:
        got = all_launches(ctx, lambda: x.slot_sum(k.evk, out=x))
        assert got[zk.PROF_BFV_KEY_SWITCH_WIDE] == 0 and got[zk.PROF_BFV_GALOIS] == 2 * len(k.elements) and got[RNS_NTT] == 0


# ---- 4. a chain from the box to the slot sum without the host --------------------------------------------------------------------

def test_chain_from_the_box_stays_on_the_device(ctx):
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    from oracle import circuit_ref as C
    cfgj = json.load(open(os.path.join(HERE, "golden", "bfv", "bfv_config.json")))
    prm = C.BfvParams()
    params, w = (1024, prm.Q, prm.T, prm.B), 8
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), params, zk.BfvConfig.from_pinning(cfgj), replay=True)
    B = make_ballots(ctx, pk, 1024, prm.Q, prm.T, prm.B, [(100, 0), (101, 0), (102, 0)])
    vk = pk.export_vk()
    pk.destroy()
    srs.destroy()
    sk = np.array([int(v) % prm.Q for v in B[100]["sk"][::-1]], dtype=np.uint64)
    rng = np.random.default_rng(280)
    case = Case(ctx, params, w, *grid(1024), 0x78, rng)
    weight = plaintexts(rng, params, (1,))[0]
    elements = [int(g) for g in zk.bfv_slot_sum_elements(params)]
    keys = [ctx.bfv_galois_keygen(params, sk, g, seed=b"\x79" * 32, base_bits=w) for g in elements]
    gk0, gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    key = B[100]["words"][:2]
    items = [(B[s]["inst"], B[s]["proof"]) for s in (100, 101, 102)]
    with zk.BallotBox(ctx, vk, params, key[0], key[1], n_groups=3) as box, case.bsgs_plan(ctx) as plan, \
            ctx.bfv_evk(params, w, elements=elements, gk0=gk0, gk1=gk1) as evk:
        assert box.add(items, [0, 2, 0]) == [(zk.BALLOT_COUNTED, "")] * 3
        c0, c1, _ = box.tally()
        h0, h1 = ctx.bfv_mul_plain(params, c0, c1, weight)
        h0, h1 = plan.apply(h0, h1)
        want = ctx.bfv_slot_sum(params, h0, h1, gk0, gk1, base_bits=w)
        x, _ = box.tally_cts()
        with x:
            x.mul_plain(weight, out=x)
            plan.apply_cts(ctx, x, out=x)
            x.slot_sum(evk, out=x)
            got = x.download()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(ctx.bfv_decrypt(params, sk, *got), ctx.bfv_decrypt(params, sk, *want))


# ---- 5. a second context ---------------------------------------------------------------------------------------------------------

def test_a_second_context_of_the_device_may_use_a_set(ctx, keysets):
    import zk_fhe_amd as zk
    k = keysets(K13, 8)
    a = pair(np.random.default_rng(290), K13, 3)
    want = ctx.bfv_slot_sum(K13, *a, k.gk0, k.gk1, base_bits=8)
    ctx2 = zk.Context(0)
    try:
        with ctx2.bfv_cts(K13, *a) as x, x.slot_sum(k.evk, ctx=ctx2) as out:
            assert same(out, want)
        with ctx.bfv_cts(K13, *a) as x, x.mul_evk(x, k.evk, ctx=ctx2) as out:
            assert same(out, ctx.bfv_mul(K13, *a, *a, *k.rlk, base_bits=8))
    finally:
        ctx2.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_calls_refuse_and_leave_dst_alone(ctx, keysets):
    import zk_fhe_amd as zk
    params, w = K13, 8
    n = params[0]
    k = keysets(params, w)
    other = (1024, Q29, 5, 19)
    rng = np.random.default_rng(300)
    a, b, d, d2, six = pair(rng, params, 3), pair(rng, params, 3), pair(rng, params, 3), pair(rng, params, 2), pair(rng, params, 6)
    m = plaintexts(rng, params, (2,))
    with ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y, ctx.bfv_cts(params, *d) as dst, ctx.bfv_cts(params, *d2) as two, \
            ctx.bfv_cts(params, *six) as x6, ctx.bfv_cts(other, *a) as alien, ctx.bfv_evk(params, w, rlk=k.rlk) as no_galois, \
            ctx.bfv_evk(params, w, elements=[5], gk0=k.gk0[:1], gk1=k.gk1[:1]) as only5, \
            ctx.bfv_evk(other, w, rlk=k.rlk, elements=k.elements, gk0=k.gk0, gk1=k.gk1) as alien_keys:
        def refused(text, fn, holder=dst, held=d):
            with pytest.raises(zk.ZkfheError, match=text):
                fn()
            assert same(holder, held), text

        for name, call in [("mul_evk", lambda e, o: x.mul_evk(y, e, out=o)), ("apply_galois_evk", lambda e, o: x.apply_galois_evk(5, e, out=o)),
                           ("slot_sum", lambda e, o: x.slot_sum(e, out=o)), ("dot", lambda e, o: x.dot(y, 1, e, out=o))]:
            refused("bfv_cts_%s: the key set and the batch have different parameters" % name, lambda: call(alien_keys, dst))
            refused("bfv_cts_%s: the batches have different parameters" % name, lambda: call(k.evk, alien), alien, a)
            # dst's count is the n_groups of dot, so there it is a that does not fit
            count = "a holds 3 ciphertexts and the call needs 2" if name == "dot" else "dst holds 2 ciphertexts and the call needs 3"
            refused("bfv_cts_%s: %s" % (name, count), lambda: call(k.evk, two), two, d2)
        refused("bfv_cts_mul_evk: b holds 2 ciphertexts and the call needs 3", lambda: x.mul_evk(two, k.evk, out=dst))
        refused("bfv_cts_mul_evk: the key set has no relinearization key", lambda: x.mul_evk(y, only5, out=dst))
        refused("bfv_cts_dot: the key set has no relinearization key", lambda: x.dot(y, 1, only5, out=dst))
        refused("bfv_cts_apply_galois_evk: the key set has no key for the Galois element 25", lambda: x.apply_galois_evk(25, only5, out=dst))
        refused("bfv_cts_apply_galois_evk: the key set has no key for the Galois element 5", lambda: x.apply_galois_evk(5, no_galois, out=dst))
        refused("bfv_cts_slot_sum: the key set has no key for the Galois element 25", lambda: x.slot_sum(only5, out=dst))
        refused("bfv_cts_apply_galois_evk: the Galois element g must be odd and below 2N", lambda: x.apply_galois_evk(4, k.evk, out=dst))
        refused("bfv_cts_apply_galois_evk: the Galois element g must be odd and below 2N", lambda: x.apply_galois_evk(2 * n + 1, k.evk, out=dst))
        # the shapes of the inner products: dst's count is n_groups
        refused("bfv_cts_dot: a holds 6 ciphertexts and the call needs 9", lambda: x6.dot(y, 3, k.evk, out=dst))
        refused("bfv_cts_dot: b holds 3 ciphertexts and the call needs 6", lambda: x6.dot(y, 2, k.evk, out=dst))
        refused("bfv_cts_dot_plain: a holds 6 ciphertexts and the call needs 9", lambda: x6.dot_plain(np.stack([m[0]] * 3), 3, out=dst))
        with ctx.bfv_cts(params, *a) as src:
            refused("bfv_cts_dot: dst must not be a source", lambda: src.dot(y, 1, k.evk, out=src), src, a)
            refused("bfv_cts_dot: dst must not be a source", lambda: x.dot(src, 1, k.evk, out=src), src, a)
            refused("bfv_cts_dot_plain: dst must not be a source", lambda: src.dot_plain(m[:1], 1, out=src), src, a)
        f = ctx.lib.zkfhe_bfv_cts_dot_plain   # two weight groups for three groups: the Python wrapper passes what it is given
        assert f(ctx.h, x.h, 1, 2, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dst.h) != 0 and same(dst, d)
        assert ctx.lib.zkfhe_last_error(ctx.h).decode() == "bfv_cts_dot_plain: m_groups must be 1 or n_groups"
        wide = m[:1].copy()
        wide[0, 3] = params[2] // 2 + 1   # the first value past the plaintext range
        refused("bfv_cts_dot_plain: a plaintext coefficient is outside", lambda: x.dot_plain(wide, 1, out=dst))
        assert same(x, a) and same(y, b)


def test_n_terms_above_the_limit_is_refused_with_the_text_of_bfv_dot(ctx):
    """Q just below 2^63 at N = 32768, where the five primes hold the fewest terms; the operands are batches of zeros, made on the
    device"""
    import zk_fhe_amd as zk
    params, w = (32768, (1 << 63) - 25, 65537, 19), 32
    limit = zk.bfv_dot_max_terms(params)
    assert limit < 2048
    sk = ctx.bfv_fhe_keypair(params, b"\x7a" * 32)[0]
    rlk = ctx.bfv_relin_keygen(params, sk, b"\x7b" * 32, base_bits=w)
    d = pair(np.random.default_rng(310), params, 1)
    with ctx.bfv_evk(params, w, rlk=rlk) as evk, ctx.bfv_cts_zeros(params, limit + 1) as x, ctx.bfv_cts(params, *d) as dst:
        with pytest.raises(zk.ZkfheError, match="bfv_cts_dot: n_terms %d is above the limit %d of zkfhe_bfv_dot_max_terms" % (limit + 1, limit)):
            x.dot(x, limit + 1, evk, out=dst)
        assert same(dst, d)
        m = np.zeros((1, params[0]), dtype=np.uint64)
        with pytest.raises(zk.ZkfheError, match="bfv_cts_dot_plain: a holds %d ciphertexts and the call needs 1" % (limit + 1)):
            x.dot_plain(m, 1, out=dst)
        assert same(dst, d)


def test_create_refuses(ctx, keysets):
    import zk_fhe_amd as zk
    params, w = K13, 8
    q = params[1]
    k = keysets(params, w)
    two0, two1 = k.gk0[:2], k.gk1[:2]
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: the Galois element 5 is repeated"):
        ctx.bfv_evk(params, w, elements=[5, 5], gk0=two0, gk1=two1)
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: the Galois element g must be odd and below 2N"):
        ctx.bfv_evk(params, w, elements=[5, 6], gk0=two0, gk1=two1)
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: the Galois element g must be odd and below 2N"):
        ctx.bfv_evk(params, w, elements=[5, 2 * params[0] + 1], gk0=two0, gk1=two1)
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: base_bits"):
        ctx.bfv_evk(params, 0, rlk=k.rlk)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        ctx.bfv_evk((1024, Q29, Q29, 19), w, rlk=k.rlk)
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: neither a relinearization key nor a Galois key"):
        ctx.bfv_evk(params, w)
    # a key word equal to Q: the last word of the last key, and of the relinearization key
    bad = k.gk1.copy()
    bad[-1, -1, -1] = q
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: a Galois-key coefficient is not below Q"):
        ctx.bfv_evk(params, w, k.rlk, k.elements, k.gk0, bad)
    bad_rlk = k.rlk[1].copy()
    bad_rlk[-1, -1] = q
    with pytest.raises(zk.ZkfheError, match="bfv_evk_create: a relinearization-key coefficient is not below Q"):
        ctx.bfv_evk(params, w, (k.rlk[0], bad_rlk), k.elements, k.gk0, k.gk1)
    bad[-1, -1, -1] = q - 1
    with ctx.bfv_evk(params, w, k.rlk, k.elements, k.gk0, bad) as ok:   # Q - 1 is a residue
        assert ok.info()["elements"] == k.elements
    # the C call: *out is NULL after a refusal
    f = ctx.lib.zkfhe_bfv_evk_create
    u64p = ctypes.POINTER(ctypes.c_uint64)
    out = ctypes.c_void_p(1)
    g = np.array([5, 5], dtype=np.uint64)
    assert f(ctx.h, ctypes.byref(zk.BfvParamsC(*params)), w, None, None, 2, *[a.ctypes.data_as(u64p) for a in (g, two0, two1)], ctypes.byref(out)) != 0
    assert out.value is None
    out = ctypes.c_void_p(1)   # one half of the relinearization key alone
    assert f(ctx.h, ctypes.byref(zk.BfvParamsC(*params)), w, k.rlk[0].ctypes.data_as(u64p), None, 0, None, None, None, ctypes.byref(out)) != 0
    assert out.value is None and ctx.lib.zkfhe_last_error(ctx.h).decode() == "bfv_evk_create: a NULL argument or a zero count"
