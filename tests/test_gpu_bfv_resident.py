"""Resident ciphertext batches on the GPU (bfv_resident.hip): the round trip, the device check of upload and store, every evaluation
call on batches bit for bit against the host-array call on the same inputs (n = 1, n = 3, and 65 ciphertexts at N = 32768, where
chunk_polys(N) + 1 makes a chunk boundary and a ragged last chunk), with the destination aliasing a source, select and sum against
numpy and bfv_sum, a chain that never visits the host against the host-array chain and its decryption, the ballot box's tally as a
batch, the launch counts per profiling slot, and the refusals.  The reference of every value is a host-array call or numpy.
Run on the MI355X box: pytest -m gpu."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.test_bfv_eval_host import Q29, Q60
from tests.test_gpu_bfv_ballot import make_ballots
from tests.test_gpu_bfv_bsgs import grid
from tests.test_gpu_bfv_eval import random_residues
from tests.test_gpu_bfv_plan import Case, plaintexts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P8 = (8, Q29, 7, 19)            # the smallest N
K13 = (1024, Q29, 7, 19)        # the k = 13 parameters
P4096 = (4096, Q60, 65537, 19)
BIG = (32768, Q60, 65537, 19)   # chunk_polys(N) = 64
CROSS = 65                      # ciphertexts: one chunk of 64 and a ragged one of 1
SMALL = [P8, K13, P4096]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def pair(rng, params, count):
    """count ciphertexts of random residues: (c0, c1), each (count, N)"""
    return random_residues(rng, (count, params[0]), params[1]), random_residues(rng, (count, params[0]), params[1])


def same(batch, want):
    got = batch.download()
    return len(want) == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def big(ctx):
    """the 65 ciphertexts of the chunk crossing, two operands, made once and never written"""
    rng = np.random.default_rng(65)
    a, b = pair(rng, BIG, CROSS), pair(rng, BIG, CROSS)
    for x in a + b:
        x.setflags(write=False)
    return a, b


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,count", [(P8, 1), (P8, 5), (K13, 3), (P4096, 3), (BIG, CROSS)])
def test_round_trip(ctx, params, count, big):
    import zk_fhe_amd as zk
    n = params[0]
    c0, c1 = big[0] if params is BIG else pair(np.random.default_rng(count), params, count)
    with ctx.bfv_cts(params, c0, c1) as cts:
        assert isinstance(cts, zk.BfvCiphertexts) and len(cts) == count
        assert cts.info() == {"params": params, "n": count, "device_bytes": 16 * count * n}
        assert same(cts, (c0, c1))
        for first, k in [(0, 1), (count - 1, 1), (count // 2, count - count // 2), (0, count)]:   # the last ciphertext alone, too
            got = cts.download(first, k)
            assert got[0].shape == (k, n) and np.array_equal(got[0], c0[first:first + k]) and np.array_equal(got[1], c1[first:first + k])
        with pytest.raises(zk.ZkfheError, match="bfv_cts_download: the range is not inside the batch"):
            cts.download(1, count)
    with ctx.bfv_cts_zeros(params, count) as z:
        assert z.info()["n"] == count
        got = z.download()
        assert got[0].shape == (count, n) and not got[0].any() and not got[1].any()
    assert cts.h is None
    with pytest.raises(zk.ZkfheError, match="closed"):
        cts.download()


def test_store_overwrites_a_range(ctx):
    params, count = K13, 5
    rng = np.random.default_rng(2)
    c0, c1 = pair(rng, params, count)
    d0, d1 = pair(rng, params, 2)
    with ctx.bfv_cts(params, c0, c1) as cts:
        cts.store(d0, d1, first=3)
        assert same(cts, (np.concatenate([c0[:3], d0]), np.concatenate([c1[:3], d1])))
        cts.store(c0[:1], c1[:1], first=4)
        assert same(cts, (np.concatenate([c0[:3], d0[:1], c0[:1]]), np.concatenate([c1[:3], d1[:1], c1[:1]])))


# ---- 2. the device check of upload and store -------------------------------------------------------------------------------------

def bad_cases():
    yield "word 0 of c0", P8, 3, 0, 0, 0
    yield "the last word of c1", K13, 3, 1, 2, K13[0] - 1
    yield "the first word past a chunk boundary", BIG, CROSS, 0, 64, 0


@pytest.mark.parametrize("what,params,count,comp,ct,word", list(bad_cases()), ids=[c[0] for c in bad_cases()])
def test_upload_refuses_a_word_equal_to_q(ctx, what, params, count, comp, ct, word, big):
    import zk_fhe_amd as zk
    q = params[1]
    src = big[0] if params is BIG else pair(np.random.default_rng(7), params, count)
    planes = [src[0].copy(), src[1].copy()]
    planes[comp][ct, word] = q
    with pytest.raises(zk.ZkfheError, match="bfv_cts_upload: a ciphertext coefficient >= Q"):
        ctx.bfv_cts(params, *planes)
    f = ctx.lib.zkfhe_bfv_cts_upload   # the C call: *out is NULL
    u64p = ctypes.POINTER(ctypes.c_uint64)
    out = ctypes.c_void_p(1)
    assert f(ctx.h, ctypes.byref(zk.BfvParamsC(*params)), count, planes[0].ctypes.data_as(u64p), planes[1].ctypes.data_as(u64p), ctypes.byref(out)) != 0
    assert out.value is None
    # a refused store leaves the batch's old contents
    with ctx.bfv_cts(params, *src) as cts:
        with pytest.raises(zk.ZkfheError, match="bfv_cts_store: a ciphertext coefficient >= Q"):
            cts.store(planes[0], planes[1])
        assert same(cts, src)
        planes[comp][ct, word] = q - 1
        cts.store(planes[0], planes[1])
        assert same(cts, planes)


@pytest.mark.parametrize("params", [P8, P4096])
def test_upload_accepts_q_minus_one_everywhere(ctx, params):
    top = np.full((3, params[0]), params[1] - 1, dtype=np.uint64)
    with ctx.bfv_cts(params, top, top) as cts:
        assert same(cts, (top, top))


# ---- 3. every evaluation call against the host-array call ------------------------------------------------------------------------

def check_call(ctx, params, sources, host, call):
    """sources: one or two (c0, c1) operands; host(*arrays) -> (out0, out1); call(*batches, out) -> a batch.  A fresh destination,
    then the destination aliasing each source in turn: the same bits, and a source that is not the destination is unchanged."""
    want = host(*[x for s in sources for x in s])
    batches = [ctx.bfv_cts(params, *s) for s in sources]
    try:
        with call(*batches, None) as out:
            assert out.info()["n"] == sources[0][0].shape[0] and same(out, want)
        assert all(same(b, s) for b, s in zip(batches, sources))
        with ctx.bfv_cts(params, *sources[-1]) as given:   # a given destination that is no source, holding other data
            assert call(*batches, given) is given and same(given, want)
        for k in range(len(sources)):
            with ctx.bfv_cts(params, *sources[k]) as dst:
                ops = batches[:k] + [dst] + batches[k + 1:]
                assert call(*ops, dst) is dst and same(dst, want), k
            assert all(same(b, s) for b, s in zip(batches, sources)), k
    finally:
        for b in batches:
            b.close()


def shapes():
    for params in SMALL:
        for count in (1, 3):
            yield params, count


@pytest.mark.parametrize("params,count", list(shapes()))
@pytest.mark.parametrize("subtract", [False, True])
def test_add_and_sub(ctx, params, count, subtract):
    rng = np.random.default_rng(31 + count)
    a, b = pair(rng, params, count), pair(rng, params, count)
    host = lambda a0, a1, b0, b1: ctx.bfv_add(params, a0, a1, b0, b1, subtract=subtract)  # noqa: E731
    call = (lambda x, y, out: x.sub(y, out=out)) if subtract else (lambda x, y, out: x.add(y, out=out))
    check_call(ctx, params, [a, b], host, call)


def test_add_across_a_chunk(ctx, big):
    a, b = big
    check_call(ctx, BIG, [a, b], lambda a0, a1, b0, b1: ctx.bfv_add(BIG, a0, a1, b0, b1), lambda x, y, out: x.add(y, out=out))
    # the same batch on both sides and as the destination: 2 a
    with ctx.bfv_cts(BIG, *a) as x:
        assert x.add(x, out=x) is x and same(x, ctx.bfv_add(BIG, *a, *a))


@pytest.mark.parametrize("params,count", list(shapes()))
@pytest.mark.parametrize("op", ["add_plain", "mul_plain"])
def test_plaintext_calls(ctx, params, count, op):
    rng = np.random.default_rng(33 + count)
    a = pair(rng, params, count)
    for m_count in sorted({1, count}):
        m = plaintexts(rng, params, (m_count,))
        m = m[0] if m_count == 1 else m
        host = lambda c0, c1: getattr(ctx, "bfv_" + op)(params, c0, c1, m)  # noqa: E731
        check_call(ctx, params, [a], host, lambda x, out: getattr(x, op)(m, out=out))
    # one plaintext per ciphertext at n = 1 is the shared plaintext's result
    if count == 3:
        m = plaintexts(rng, params, (3,))
        check_call(ctx, params, [a], lambda c0, c1: getattr(ctx, "bfv_" + op)(params, c0, c1, m), lambda x, out: getattr(x, op)(m, out=out))


@pytest.mark.parametrize("op", ["add_plain", "mul_plain"])
def test_plaintext_calls_across_a_chunk(ctx, big, op):
    """one plaintext per ciphertext: the second chunk's plaintexts are uploaded from their own offset, into a fresh destination and
    in place"""
    a, _ = big
    m = plaintexts(np.random.default_rng(34), BIG, (CROSS,))
    want = getattr(ctx, "bfv_" + op)(BIG, *a, m)
    with ctx.bfv_cts(BIG, *a) as x:
        with getattr(x, op)(m) as out:
            assert same(out, want) and same(x, a)
        assert getattr(x, op)(m, out=x) is x and same(x, want)


def relin_key(ctx, params, w, seed):
    sk = ctx.bfv_fhe_keypair(params, bytes([seed]) * 32)[0]
    return sk, ctx.bfv_relin_keygen(params, sk, bytes([seed + 1]) * 32, base_bits=w)


@pytest.mark.parametrize("params,w,count", [(P8, 16, 1), (P8, 16, 3), (K13, 8, 1), (K13, 8, 3), (P4096, 16, 1), (P4096, 16, 3)])
def test_mul(ctx, params, w, count):
    rng = np.random.default_rng(35 + count)
    _, (rlk0, rlk1) = relin_key(ctx, params, w, 0x51)
    a, b = pair(rng, params, count), pair(rng, params, count)
    host = lambda a0, a1, b0, b1: ctx.bfv_mul(params, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)  # noqa: E731
    check_call(ctx, params, [a, b], host, lambda x, y, out: x.mul(y, rlk0, rlk1, base_bits=w, out=out))


def test_mul_across_a_chunk(ctx, big):
    a, b = big
    w = 32
    _, (rlk0, rlk1) = relin_key(ctx, BIG, w, 0x53)
    host = lambda a0, a1, b0, b1: ctx.bfv_mul(BIG, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)  # noqa: E731
    check_call(ctx, BIG, [a, b], host, lambda x, y, out: x.mul(y, rlk0, rlk1, base_bits=w, out=out))


@pytest.mark.parametrize("params,count", list(shapes()))
def test_apply_galois(ctx, params, count):
    rng = np.random.default_rng(37 + count)
    n, w = params[0], 8 if params is K13 else 16
    sk = ctx.bfv_fhe_keypair(params, b"\x55" * 32)[0]
    a = pair(rng, params, count)
    for g in (5, 2 * n - 1):
        gk0, gk1 = ctx.bfv_galois_keygen(params, sk, g, seed=b"\x56" * 32, base_bits=w)
        host = lambda c0, c1: ctx.bfv_apply_galois(params, c0, c1, g, gk0, gk1, base_bits=w)  # noqa: E731
        check_call(ctx, params, [a], host, lambda x, out: x.apply_galois(g, gk0, gk1, base_bits=w, out=out))


@pytest.fixture(scope="module")
def plans(ctx):
    """one flat and one two-level plan at N = 1024 over three elements (3 x 3 for the two-level one)"""
    rng = np.random.default_rng(39)
    case = Case(ctx, K13, 8, *grid(K13[0]), 0x58, rng)
    flat, bsgs = case.flat_plan(ctx), case.bsgs_plan(ctx)
    yield case, flat, bsgs
    flat.close()
    bsgs.close()


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("two_level", [False, True])
def test_plan_apply(ctx, plans, count, two_level):
    case, flat, bsgs = plans
    plan = bsgs if two_level else flat
    a = pair(np.random.default_rng(41 + count), K13, count)
    check_call(ctx, K13, [a], lambda c0, c1: plan.apply(c0, c1), lambda x, out: plan.apply_cts(ctx, x, out=out))
    with ctx.bfv_cts(K13, *a) as x:   # and the host-array call that the plan stands for
        want = (case.bsgs_call if two_level else case.flat_call)(ctx, *a)
        with plan.apply_cts(None, x) as out:
            assert same(out, want)


# ---- 4. select -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", SMALL)
def test_select(ctx, params):
    import zk_fhe_amd as zk
    count = 4
    c0, c1 = pair(np.random.default_rng(43), params, count)
    with ctx.bfv_cts(params, c0, c1) as cts:
        for idx in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 2, 0], [1], [count - 1], [0] * 9):
            with cts.select(idx) as out:
                assert out.info()["n"] == len(idx) and same(out, (c0[idx], c1[idx])), idx
        assert same(cts, (c0, c1))
        with ctx.bfv_cts_zeros(params, 2) as dst:
            assert cts.select([3, 1], out=dst) is dst and same(dst, (c0[[3, 1]], c1[[3, 1]]))
            with pytest.raises(zk.ZkfheError, match="bfv_cts_select: an index is not below the source's count"):
                cts.select([0, count], out=dst)
            with pytest.raises(zk.ZkfheError, match="bfv_cts_select: dst holds 2 ciphertexts and the call needs 3"):
                cts.select([0, 1, 2], out=dst)
            assert same(dst, (c0[[3, 1]], c1[[3, 1]]))
        with pytest.raises(zk.ZkfheError, match="bfv_cts_select: dst must not be the source"):
            cts.select([3, 2, 1, 0], out=cts)
        assert same(cts, (c0, c1))


def test_select_across_a_chunk(ctx, big):
    c0, c1 = big[0]
    idx = [64, 0, 63, 64]
    with ctx.bfv_cts(BIG, c0, c1) as cts, cts.select(idx) as out:
        assert same(out, (c0[idx], c1[idx]))


# ---- 5. sum ----------------------------------------------------------------------------------------------------------------------

def host_group_sums(ctx, params, c0, c1, groups, n_groups):
    """per group the bfv_sum of its members; an empty group is zeros"""
    out0, out1 = (np.zeros((n_groups, params[0]), dtype=np.uint64) for _ in range(2))
    for g in range(n_groups):
        members = [j for j, x in enumerate(groups) if x == g]
        if members:
            out0[g], out1[g] = ctx.bfv_sum(params, c0[members], c1[members])
    return out0, out1


@pytest.mark.parametrize("params", SMALL)
def test_sum(ctx, params):
    import zk_fhe_amd as zk
    n, q = params[0], params[1]
    c0, c1 = pair(np.random.default_rng(45), params, 5)
    with ctx.bfv_cts(params, c0, c1) as cts:
        with cts.sum() as total:
            s0, s1 = ctx.bfv_sum(params, c0, c1)
            assert total.info()["n"] == 1 and same(total, (s0[None], s1[None]))
        groups = [0, 2, 2, -1, 0]
        with cts.sum(groups, 3) as out:
            want = host_group_sums(ctx, params, c0, c1, groups, 3)
            assert same(out, want)
            assert not want[0][1].any() and not want[1][1].any()                       # group 1 is empty
            with out.select([0]) as g0:
                assert same(g0, ctx_sum_rows(ctx, params, c0, c1, [0, 4]))             # the skipped member 3 is left out
        with ctx.bfv_cts_zeros(params, 3) as dst:
            with pytest.raises(zk.ZkfheError, match="bfv_cts_sum: a group is not below n_groups"):
                cts.sum([0, 1, 2, 3, 0], 3, out=dst)
            got = dst.download()
            assert not got[0].any() and not got[1].any()
        with pytest.raises(zk.ZkfheError, match="bfv_cts_sum: n_groups must be in"):
            cts.sum(None, 4097)
        with ctx.bfv_cts(params, c0, c1) as five:
            with pytest.raises(zk.ZkfheError, match="bfv_cts_sum: dst must not be the source"):
                five.sum([0, 1, 2, 3, 4], 5, out=five)
            assert same(five, (c0, c1))
    # all Q - 1: every addition wraps
    top = np.full((5, n), q - 1, dtype=np.uint64)
    with ctx.bfv_cts(params, top, top) as cts, cts.sum() as total:
        want = np.full((1, n), (5 * (q - 1)) % q, dtype=np.uint64)
        assert same(total, (want, want)) and same(total, [x[None] for x in ctx.bfv_sum(params, top, top)])


def ctx_sum_rows(ctx, params, c0, c1, rows):
    s0, s1 = ctx.bfv_sum(params, c0[rows], c1[rows])
    return s0[None], s1[None]


def test_sum_across_a_chunk(ctx, big):
    c0, c1 = big[0]
    groups = [j % 2 for j in range(CROSS)]
    groups[64] = 0   # the ragged chunk's ciphertext
    with ctx.bfv_cts(BIG, c0, c1) as cts, cts.sum(groups, 2) as out:
        assert same(out, host_group_sums(ctx, BIG, c0, c1, groups, 2))


# ---- 6. a chain without the host -------------------------------------------------------------------------------------------------

def test_chain_stays_on_the_device(ctx):
    import zk_fhe_amd as zk
    params, w, count = (1024, Q60, 12289, 19), 8, 2
    n, t = params[0], params[2]
    rng = np.random.default_rng(47)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x5a" * 32)
    values = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    weights = rng.integers(0, t, size=n, dtype=np.uint64)
    ct = ctx.bfv_encrypt(params, pk0, pk1, ctx.bfv_encode_slots(params, values), b"\x5b" * 32)
    weight = ctx.bfv_encode_slots(params, weights)[0]
    elements = [int(g) for g in zk.bfv_slot_sum_elements(params)]
    keys = [ctx.bfv_galois_keygen(params, sk, g, seed=b"\x5c" * 32, base_bits=w) for g in elements]
    gk0, gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    # the host-array chain: what the header defines the slot sum as
    h0, h1 = ctx.bfv_mul_plain(params, ct["c0"], ct["c1"], weight)
    want = ctx.bfv_slot_sum(params, h0, h1, gk0, gk1, base_bits=w)
    with ctx.bfv_cts(params, ct["c0"], ct["c1"]) as x, ctx.bfv_cts_zeros(params, count) as rot:
        x.mul_plain(weight, out=x)
        for g, (k0, k1) in zip(elements, keys):
            x.apply_galois(g, k0, k1, base_bits=w, out=rot)
            x.add(rot, out=x)
        got = x.download()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    slots = ctx.bfv_decode_slots(params, ctx.bfv_decrypt(params, sk, got[0], got[1]))
    for j in range(count):
        total = sum(int(v) * int(u) for v, u in zip(values[j], weights)) % t
        assert [int(s) for s in slots[j]] == [total] * n, j


# ---- 7. the box ------------------------------------------------------------------------------------------------------------------

def test_box_tally_as_a_batch(ctx):
    """three k = 13 proofs into three groups, of which group 1 stays empty"""
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    from oracle import circuit_ref as C
    cfgj = json.load(open(os.path.join(HERE, "golden", "bfv", "bfv_config.json")))
    prm = C.BfvParams()
    params = (1024, prm.Q, prm.T, prm.B)
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), params, zk.BfvConfig.from_pinning(cfgj), replay=True)
    B = make_ballots(ctx, pk, 1024, prm.Q, prm.T, prm.B, [(100, 0), (101, 0), (102, 0)])
    vk = pk.export_vk()
    pk.destroy()
    srs.destroy()
    key = B[100]["words"][:2]
    items = [(B[s]["inst"], B[s]["proof"]) for s in (100, 101, 102)]
    with zk.BallotBox(ctx, vk, params, key[0], key[1], n_groups=3) as box:
        assert box.add(items, [0, 2, 0]) == [(zk.BALLOT_COUNTED, "")] * 3
        c0, c1, counted = box.tally()
        cts, counted_cts = box.tally_cts()
        with cts:
            assert cts.info()["n"] == 3 and cts.params == params
            assert same(cts, (c0, c1)) and np.array_equal(counted_cts, counted) and list(counted) == [2, 0, 1]
            assert not c0[1].any() and c0[0].any() and c0[2].any()
            # the box is unchanged: the same tally again, into the batch given
            again, counted_again = box.tally_cts(out=cts)
            assert again is cts and same(cts, (c0, c1)) and np.array_equal(counted_again, counted)
        after = box.tally()
        assert all(np.array_equal(a, b) for a, b in zip(after, (c0, c1, counted))) and box.totals["counted"] == 3
        with ctx.bfv_cts_zeros(params, 2) as two:
            with pytest.raises(zk.ZkfheError, match="bfv_cts_box_tally: dst holds 2 ciphertexts and the call needs 3"):
                box.tally_cts(out=two)
        with ctx.bfv_cts_zeros(K13[:2] + (5, 19), 3) as other:
            with pytest.raises(zk.ZkfheError, match="bfv_cts_box_tally: the box and the batch have different parameters"):
                box.tally_cts(out=other)


# ---- 8. the same kernels ---------------------------------------------------------------------------------------------------------

def launches(ctx, fn):
    """the launch count of every profiling slot over fn()"""
    import zk_fhe_amd as zk
    ctx.prof_enable(True)   # resets the slots
    try:
        fn()
        return [ctx.prof_read(slot)["launches"] for slot in range(zk.PROF_BFV_RESIDENT + 1)]
    finally:
        ctx.prof_enable(False)


def test_batch_calls_launch_the_kernels_of_the_host_array_calls(ctx, plans):
    import zk_fhe_amd as zk
    params, w = K13, 8
    _, (rlk0, rlk1) = relin_key(ctx, params, w, 0x5d)
    rng = np.random.default_rng(49)
    a, b = pair(rng, params, 3), pair(rng, params, 3)
    _, flat, bsgs = plans
    with ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y, ctx.bfv_cts_zeros(params, 3) as out:
        for host, call in [(lambda: ctx.bfv_mul(params, *a, *b, rlk0, rlk1, base_bits=w), lambda: x.mul(y, rlk0, rlk1, base_bits=w, out=out)),
                           (lambda: flat.apply(*a), lambda: flat.apply_cts(ctx, x, out=out)),
                           (lambda: bsgs.apply(*a), lambda: bsgs.apply_cts(ctx, x, out=out))]:
            want, got = launches(ctx, host), launches(ctx, call)
            assert sum(want) > 0 and want[zk.PROF_BFV_RESIDENT] == 0
            assert got == want
    up = launches(ctx, lambda: ctx.bfv_cts(params, *a).close())
    assert up[zk.PROF_BFV_RESIDENT] == 1 and sum(up) == 1


# ---- 9. mismatches ---------------------------------------------------------------------------------------------------------------

def test_mismatches_are_refused_and_leave_dst_alone(ctx):
    import zk_fhe_amd as zk
    params, w = K13, 8
    n, q, t = params[0], params[1], params[2]
    other = (1024, Q29, 5, 19)
    rng = np.random.default_rng(51)
    a, b, d = pair(rng, params, 3), pair(rng, params, 3), pair(rng, params, 3)
    d2 = pair(rng, params, 2)
    _, (rlk0, rlk1) = relin_key(ctx, params, w, 0x5f)
    m = plaintexts(rng, params, (1,))[0]
    with ctx.bfv_cts(params, *a) as x, ctx.bfv_cts(params, *b) as y, ctx.bfv_cts(params, *d) as dst, ctx.bfv_cts(params, *d2) as two, \
            ctx.bfv_cts(other, *a) as alien:
        def refused(text, fn, holder=dst, held=d):
            with pytest.raises(zk.ZkfheError, match=text):
                fn()
            assert same(holder, held), text

        refused("bfv_cts_add: the batches have different parameters", lambda: x.add(alien, out=dst))
        refused("bfv_cts_add: the batches have different parameters", lambda: alien.add(x, out=dst))
        refused("bfv_cts_mul: the batches have different parameters", lambda: x.mul(y, rlk0, rlk1, base_bits=w, out=alien), alien, a)
        refused("bfv_cts_add: b holds 2 ciphertexts and the call needs 3", lambda: x.add(two, out=dst))
        refused("bfv_cts_add: dst holds 2 ciphertexts and the call needs 3", lambda: x.add(y, out=two), two, d2)
        refused("bfv_cts_mul_plain: dst holds 2 ciphertexts and the call needs 3", lambda: x.mul_plain(m, out=two), two, d2)
        refused("bfv_cts_apply_galois: dst holds 2 ciphertexts and the call needs 3", lambda: x.apply_galois(5, rlk0, rlk1, base_bits=w, out=two), two, d2)
        refused("bfv_cts_mul: base_bits", lambda: x.mul(y, rlk0, rlk1, base_bits=0, out=dst))
        refused("bfv_cts_apply_galois: base_bits", lambda: x.apply_galois(5, rlk0, rlk1, base_bits=0, out=dst))
        refused("bfv_cts_apply_galois: the Galois element g must be odd and below 2N", lambda: x.apply_galois(4, rlk0, rlk1, base_bits=w, out=dst))
        wide = m.copy()
        wide[3] = t // 2 + 1   # the first value past the plaintext range
        refused("bfv_cts_mul_plain: a plaintext coefficient is outside", lambda: x.mul_plain(wide, out=dst))
        refused("bfv_cts_add_plain: a plaintext coefficient is outside", lambda: x.add_plain(wide, out=dst))
        f = ctx.lib.zkfhe_bfv_cts_add_plain   # two plaintexts for three ciphertexts: the Python wrapper would refuse the shape itself
        mm = np.stack([m, m])
        assert f(ctx.h, x.h, 2, mm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), dst.h) != 0 and same(dst, d)
        assert ctx.lib.zkfhe_last_error(ctx.h).decode() == "bfv_cts_add_plain: m_count must be 1 or the ciphertext count"
        big_key = rlk1.copy()
        big_key[-1, n - 1] = q
        refused("bfv_cts_mul: a relinearization-key coefficient is not below Q", lambda: x.mul(y, rlk0, big_key, base_bits=w, out=dst))
        refused("bfv_cts_apply_galois: a Galois-key coefficient is not below Q", lambda: x.apply_galois(5, rlk0, big_key, base_bits=w, out=dst))
        assert same(x, a) and same(y, b)
    with pytest.raises(zk.ZkfheError, match="bfv_cts_alloc: a NULL argument or a zero count"):
        ctx.bfv_cts_zeros(params, 0)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        ctx.bfv_cts_zeros((1024, Q29, Q29, 19), 1)


def test_plan_of_other_parameters_is_refused(ctx, plans):
    import zk_fhe_amd as zk
    _, flat, _ = plans
    a = pair(np.random.default_rng(53), P8, 2)
    with ctx.bfv_cts(P8, *a) as x, ctx.bfv_cts_zeros(P8, 2) as dst:
        with pytest.raises(zk.ZkfheError, match="bfv_cts_plan_apply: the plan and the batch have different parameters"):
            flat.apply_cts(ctx, x, out=dst)
        got = dst.download()
        assert not got[0].any() and not got[1].any()


def test_a_second_context_of_the_device_may_use_a_batch(ctx):
    import zk_fhe_amd as zk
    a, b = pair(np.random.default_rng(55), K13, 3), pair(np.random.default_rng(56), K13, 3)
    ctx2 = zk.Context(0)
    try:
        with ctx.bfv_cts(K13, *a) as x, ctx2.bfv_cts(K13, *b) as y:
            with x.add(y, ctx=ctx2) as out:
                assert same(out, ctx.bfv_add(K13, *a, *b))
                assert np.array_equal(out.download(ctx=ctx2)[0], out.download()[0])
    finally:
        ctx2.close()
