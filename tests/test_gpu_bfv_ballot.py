"""The ballot box on the GPU (bfv_ballot.hip): zkfhe_bfv_sum_instances bit for bit against its definition (ref_sum_instances of
tests/test_bfv_ballot_host.py) on synthetic instances -- the modular add at its edge, empty, skipped and bad groups, every malformed
shape between good items, more than one chunk, the largest N, any order -- and the box on real proofs against ref_box, bfv_sum and
the decryption: the decision order, the copy attack, repeats across calls, any split into calls, a second context.
Run on the MI355X box: pytest -m gpu."""
import json
import os
import random

import numpy as np
import pytest

from tests.test_bfv_ballot_host import make_instances, malformed, random_item, ref_box, ref_sum_instances
from tests.test_bfv_eval_host import Q29, Q60, Q63

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def check_sum(ctx, params, items, groups, n_groups):
    """the call against the oracle: sums, counts and statuses"""
    got = ctx.bfv_sum_instances(params, items, groups, n_groups)
    want = ref_sum_instances(params, items, groups, n_groups)
    assert got[0].shape == got[1].shape == (n_groups, params[0]) and got[0].dtype == np.uint64
    for g, w, what in zip(got, want, ("out0", "out1", "counted", "status")):
        assert np.array_equal(g, w), what
    return got


# ---- 1. sums straight from instance scalars ------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [Q29, Q60, Q63])
def test_sum_instances_edges_and_malformed_items(ctx, q):
    import zk_fhe_amd as zk
    params = (8, q, 7, 1)
    n = 8
    rng = random.Random(q % 1009)
    top = [q - 1] * n
    items = [make_instances(params, top, top, top, top) for _ in range(3)]   # 3 (Q - 1) mod Q: the add at its edge, twice
    groups = [0, 0, 0]
    good = random_item(rng, params)
    bad = malformed(params, good)
    assert len(bad) == 7
    for k, (name, inst) in enumerate(bad.items()):                           # each malformed item between two good ones
        items += [random_item(rng, params), inst]
        groups += [2 * (k % 2), 2 * ((k + 1) % 2)]
    items += [random_item(rng, params), random_item(rng, params), random_item(rng, params)]
    groups += [2, -1, 3]                                                      # a good one, a skipped one, a bad group
    out0, out1, counted, status = check_sum(ctx, params, items, groups, 3)
    assert not out0[1].any() and not out1[1].any() and counted[1] == 0       # group 1 is left empty
    assert list(status[:3]) == [zk.BALLOT_COUNTED] * 3 and [int(x) for x in out0[0]] != [0] * n
    assert list(status[4::2][:7]) == [zk.BALLOT_NOT_A_CIPHERTEXT] * 7
    assert list(status[-2:]) == [zk.BALLOT_SKIPPED, zk.BALLOT_BAD_GROUP]
    # the sums are those of the good items alone
    keep = [j for j in range(len(items)) if status[j] == zk.BALLOT_COUNTED]
    assert len(keep) == 3 + 7 + 1 and int(counted.sum()) == len(keep)
    alone = ref_sum_instances(params, [items[j] for j in keep], [groups[j] for j in keep], 3)
    assert np.array_equal(out0, alone[0]) and np.array_equal(out1, alone[1]) and np.array_equal(counted, alone[2])
    # three times Q - 1 alone
    e0, e1, ec, _ = check_sum(ctx, params, items[:3], None, 1)
    assert [int(x) for x in e0[0]] == [q - 3] * n == [int(x) for x in e1[0]] and int(ec[0]) == 3


def test_sum_instances_of_one_item(ctx):
    import zk_fhe_amd as zk
    params = (8, Q29, 7, 1)
    item = random_item(random.Random(2), params)
    out0, out1, counted, status = check_sum(ctx, params, [item], None, 1)
    assert [int(x) for x in out0[0]] == item[16:24] and [int(x) for x in out1[0]] == item[24:32] and list(counted) == [1]
    # and one item that is not a ciphertext: zeros, never an error
    out0, _, counted, status = check_sum(ctx, params, [item[:-1]], [0], 2)
    assert not out0.any() and list(counted) == [0, 0] and list(status) == [zk.BALLOT_NOT_A_CIPHERTEXT]
    # Instances and bytes are taken like lists of integers
    raw = b"".join(v.to_bytes(32, "little") for v in item)
    for form in (raw, zk.Instances(raw)):
        assert np.array_equal(ctx.bfv_sum_instances(params, [form])[0][0], np.array(item[16:24], dtype=np.uint64))


def test_sum_instances_across_chunks_and_in_any_order(ctx):
    """600 items at N = 8, of which 594 reach the device: more than one chunk (512 candidates; the host drops skipped items, bad
    groups, wrong counts and wrong tails before it chunks) of lists and segment offsets.  Items that only the device check can refuse
    sit on both sides of the chunk boundary, group 4 straddles it, and every group has items in both chunks."""
    import zk_fhe_amd as zk
    params = (8, Q60, 65537, 19)
    n, q, chunk = 8, Q60, 512
    rng = random.Random(6)
    items = [random_item(rng, params) for _ in range(600)]
    groups = [rng.randrange(5) for _ in range(600)]
    groups[7], groups[8] = -1, 5                                             # one skipped, one bad group
    bad = malformed(params, items[0])
    dropped = {1: "5N instances", 100: "5N + 2 instances", 300: "the leading 1 of the tail missing", 598: "constant term 2"}
    for j, name in dropped.items():
        items[j] = bad[name]
    # the candidates, as the host path of zkfhe.h picks them: a group in range, 5 N + 1 scalars, the tail of x^N + 1
    cand = [j for j in range(600) if 0 <= groups[j] < 5 and j not in dropped]
    assert len(cand) == 594 > chunk
    for k in range(chunk - 4, chunk + 4):
        groups[cand[k]] = 4
    on_device = {chunk - 2: ("a scalar equal to Q", 2 * n + 3, q), chunk - 1: ("limb 1 = 1 over a small limb 0", 3 * n + 1, (1 << 64) + 5),
                 chunk: ("limb 3 set", 4 * n - 1, (1 << 192) + 5), chunk + 1: ("a scalar equal to Q", 2 * n, q), len(cand) - 1: ("limb 3 set", 2 * n, 1 << 192)}
    for k, (_, pos, value) in on_device.items():
        items[cand[k]][pos] = value
    for g in range(5):                                                       # every group on both sides of the boundary
        assert {groups[j] for j in cand[:chunk]} >= {g} and {groups[j] for j in cand[chunk:]} >= {g}
    first = check_sum(ctx, params, items, groups, 5)
    status = first[3]
    assert [int(status[cand[k]]) for k in on_device] == [zk.BALLOT_NOT_A_CIPHERTEXT] * 5
    assert [int(status[j]) for j in dropped] == [zk.BALLOT_NOT_A_CIPHERTEXT] * 4
    assert int(status[7]) == zk.BALLOT_SKIPPED and int(status[8]) == zk.BALLOT_BAD_GROUP
    assert int(first[2].sum()) == len(cand) - len(on_device) == 589 and all(int(c) > 50 for c in first[2])
    # what the second chunk adds is there: the sums of the first chunk's kept items alone differ in every group
    head = ref_sum_instances(params, [items[j] for j in cand[:chunk]], [groups[j] for j in cand[:chunk]], 5)
    assert all(not np.array_equal(first[0][g], head[0][g]) and int(first[2][g]) > int(head[2][g]) for g in range(5))
    perm = list(range(600))
    rng.shuffle(perm)
    again = check_sum(ctx, params, [items[j] for j in perm], [groups[j] for j in perm], 5)
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(first[3][perm], again[3])


def test_sum_instances_at_the_largest_n(ctx):
    n, q = 32768, Q63
    params = (n, q, 65537, 19)
    rng = np.random.default_rng(7)
    items, words = [], []
    for _ in range(2):
        w = rng.integers(q - (1 << 40), q, 4 * n, dtype=np.uint64)          # near Q: every sum wraps
        scal = np.zeros((5 * n + 1, 4), dtype=np.uint64)
        scal[:4 * n, 0] = w
        scal[4 * n, 0] = scal[5 * n, 0] = 1
        items.append(scal.tobytes())
        words.append(w)
    out0, out1, counted, status = ctx.bfv_sum_instances(params, items)
    want = [(int(a) + int(b)) % q for a, b in zip(words[0][2 * n:], words[1][2 * n:])]
    assert [int(x) for x in out0[0]] == want[:n] and [int(x) for x in out1[0]] == want[n:]
    assert list(counted) == [2] and list(status) == [0, 0]
    # the last scalar of c1 with limb 3 set: the check reaches the end of the span
    scal = np.frombuffer(items[1], dtype=np.uint64).reshape(-1, 4).copy()
    scal[4 * n - 1, 3] = 1
    out0, out1, counted, status = ctx.bfv_sum_instances(params, [items[0], scal.tobytes()])
    assert np.array_equal(out0[0], words[0][2 * n:3 * n]) and np.array_equal(out1[0], words[0][3 * n:]) and list(status) == [0, 3]


def test_sum_instances_refusals(ctx):
    import zk_fhe_amd as zk
    params = (8, Q29, 7, 1)
    item = random_item(random.Random(3), params)
    with pytest.raises(zk.ZkfheError, match="bfv_sum_instances: a NULL argument or a zero count"):
        ctx.bfv_sum_instances(params, [])
    for n_groups in (0, 4097):
        with pytest.raises(zk.ZkfheError, match="bfv_sum_instances: n_groups"):
            ctx.bfv_sum_instances(params, [item], n_groups=n_groups)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        ctx.bfv_sum_instances((8, Q29, Q29, 1), [item])
    assert ctx.bfv_sum_instances(params, [item], n_groups=4096)[2][0] == 1


# ---- 2. the box on real proofs ---------------------------------------------------------------------------------------------------

def make_ballots(ctx, pk, n, q, t, b, seeds):
    """proofs of real encryptions (zk_fhe_amd.inputs): seed -> dict(inst, proof, m, sk, words); key_seed picks the public key"""
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    out = {}
    for seed, key_seed in seeds:
        inp, sec = inputs.generate(n, q, t, b, seed=seed, with_secret=True, key_seed=key_seed)
        proof, inst, _ = pk.prove(json.dumps(inp), b"ballot-%d" % seed)
        out[seed] = dict(inst=list(inst), proof=proof, m=sec["m"], sk=sec["sk"], words=zk.bfv_instance_words((n, q, t, b), inst))
    return out


@pytest.fixture(scope="module")
def k14(ctx):
    """the smallest circuit the GPU prover is tested on, N = 16: five ballots under key 0 and one under key 1"""
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    from oracle import circuit_ref as C
    from oracle import halo2_ref as H
    prm = C.BfvParams(N=16)
    params = (16, prm.Q, prm.T, prm.B)
    first = inputs.generate(16, prm.Q, prm.T, prm.B, seed=10, key_seed=0)
    hcfg = H.auto_config(14, 109, H.BfvCircuit(first, prm))
    srs = zk.Srs(ctx, 14)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(first), params, zk.BfvConfig(14, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 109))
    ballots = make_ballots(ctx, pk, 16, prm.Q, prm.T, prm.B, [(10, 0), (11, 0), (12, 0), (13, 0), (14, 0), (20, 1)])
    vk = pk.export_vk()
    pk.destroy()
    srs.destroy()
    return params, vk, ballots


def expect_tally(ctx, params, ballots, counted_seeds, n_groups):
    """per group: bfv_sum of exactly the counted ciphertexts' words, and the centred sum of their messages as residues mod Q"""
    n, q, t = params[0], params[1], params[2]
    c0, c1, ms = np.zeros((n_groups, n), dtype=np.uint64), np.zeros((n_groups, n), dtype=np.uint64), []
    for g in range(n_groups):
        seeds = [s for s, grp in counted_seeds if grp == g]
        if seeds:
            c0[g], c1[g] = ctx.bfv_sum(params, np.array([ballots[s]["words"][2] for s in seeds]), np.array([ballots[s]["words"][3] for s in seeds]))
        total = sum(ballots[s]["m"].astype(object) for s in seeds) if seeds else np.zeros(n, dtype=object)
        r = [int(v) % t for v in total]
        ms.append(np.array([(v - t if v > t // 2 else v) % q for v in r[::-1]], dtype=np.uint64))
    return c0, c1, ms


def test_box_decision_order_and_tally(ctx, k14):
    import zk_fhe_amd as zk
    params, vk, B = k14
    n, q = params[0], params[1]
    V, key = B[10], B[10]["words"][:2]
    assert not np.array_equal(B[20]["words"][0], key[0])                      # two public keys
    flip = bytearray(V["proof"])
    flip[len(flip) - 100] ^= 1                                                # an evaluation (scalar) byte
    forged = (V["inst"], bytes(flip))
    pair = lambda s: (B[s]["inst"], B[s]["proof"])  # noqa: E731
    items = [forged, pair(10), pair(11), pair(12), pair(13), pair(20), pair(10), pair(14)]
    groups = [0, 0, 1, 0, 1, 0, 0, 2]
    verify = lambda inst, proof: zk.bfv_verify(vk, inst, proof)  # noqa: E731
    ref = ref_box(params, key[0], key[1], 2, verify)
    box = zk.BallotBox(ctx, vk, params, key[0], key[1], n_groups=2)
    got = box.add(items, groups)
    assert got == ref.add(items, groups)
    assert got[0] == (zk.BALLOT_REJECTED, verify(*forged)[1]) and not verify(*forged)[0]
    assert got[1] == (zk.BALLOT_COUNTED, "")                                  # the forgery before it did not shut it out
    assert [s for s, _ in got[2:5]] == [zk.BALLOT_COUNTED] * 3
    assert [s for s, _ in got[5:]] == [zk.BALLOT_WRONG_KEY, zk.BALLOT_REPEATED, zk.BALLOT_BAD_GROUP]
    mid = box.tally()                                                         # between adds; the box is unchanged by it
    second = [pair(12), pair(14)]
    got2 = box.add(second, [0, 1])
    assert got2 == ref.add(second, [0, 1]) == [(zk.BALLOT_REPEATED, ""), (zk.BALLOT_COUNTED, "")]
    c0, c1, counted = box.tally()
    counted_seeds = [(10, 0), (11, 1), (12, 0), (13, 1), (14, 1)]
    want0, want1, want_m = expect_tally(ctx, params, B, counted_seeds, 2)
    assert np.array_equal(c0, want0) and np.array_equal(c1, want1) and list(counted) == [2, 3]
    for a, b in zip((c0, c1, counted), ref.tally()):
        assert np.array_equal(a, b)
    m0, m1, mc = expect_tally(ctx, params, B, counted_seeds[:4], 2)
    assert np.array_equal(mid[0], m0) and np.array_equal(mid[1], m1) and list(mid[2]) == [2, 2]
    sk = np.array([int(x) % q for x in V["sk"][::-1]], dtype=np.uint64)
    for g in range(2):
        assert np.array_equal(ctx.bfv_decrypt(params, sk, c0[g], c1[g])[0], want_m[g]), g
    totals = box.totals
    assert sum(totals.values()) == len(items) + len(second) == 10 and totals == ref.totals
    assert totals["counted"] == 5 and totals["repeated"] == 2 and totals["skipped"] == 0
    with pytest.raises(zk.ZkfheError, match="bfv_box: a NULL argument or a zero count"):
        box.add([])
    # the same ballots one per call, in reverse order, from a second context of the same device: the same tally
    ctx2 = zk.Context(0)
    try:
        box2 = zk.BallotBox(ctx, vk, params, key[0], key[1], n_groups=2)
        every = list(zip(items + second, groups + [0, 1]))[::-1]
        seen = [box2.add([it], [g], ctx=ctx2)[0][0] for it, g in every]
        assert sorted(seen) == sorted([s for s, _ in got + got2])
        assert seen[1] == zk.BALLOT_COUNTED and seen[6] == zk.BALLOT_REPEATED     # ballot 12: the other copy is flagged now
        for a, b in zip(box2.tally(ctx=ctx2), (c0, c1, counted)):
            assert np.array_equal(a, b)
        assert box2.totals == totals
        box2.close()
    finally:
        ctx2.close()
    # the group plays no part in what a repeat is: ballot 11 was counted in group 1
    assert box.add([pair(11)], [0]) == ref.add([pair(11)], [0]) == [(zk.BALLOT_REPEATED, "")]
    assert np.array_equal(box.tally()[0], c0) and box.totals["repeated"] == 3
    box.close()
    with pytest.raises(zk.ZkfheError, match="closed"):                        # the Python object refuses; the C call is not attempted
        box.tally()


def test_box_checks_residues_after_the_proof(ctx, k14):
    """Step 5 of the order.  A proof knows nothing of the box's parameters, so a box made with a Q just above the key's largest
    coefficient accepts the proof of ballot 11 and its device check then finds the ciphertext coefficient that is not below that Q."""
    import zk_fhe_amd as zk
    params, vk, B = k14
    key = B[10]["words"][:2]
    k_max = max(int(key[0].max()), int(key[1].max()))
    with pytest.raises(zk.ZkfheError, match="bfv_box: a public-key coefficient is not below Q"):
        zk.BallotBox(ctx, vk, (16, k_max, 7, 1), key[0], key[1])
    with pytest.raises(zk.ZkfheError, match="bfv_box: n_groups"):
        zk.BallotBox(ctx, vk, params, key[0], key[1], n_groups=4097)
    assert max(int(B[11]["words"][2].max()), int(B[11]["words"][3].max())) > k_max      # what the case rests on
    assert max(int(B[12]["words"][2].max()), int(B[12]["words"][3].max())) < k_max
    with zk.BallotBox(ctx, vk, (16, k_max + 1, 7, 1), key[0], key[1]) as box:
        got = box.add([(B[12]["inst"], B[12]["proof"]), (B[11]["inst"], B[11]["proof"])])
        assert got == [(zk.BALLOT_COUNTED, ""), (zk.BALLOT_NOT_A_CIPHERTEXT, "")]
        c0, c1, counted = box.tally()
        assert np.array_equal(c0[0], B[12]["words"][2]) and np.array_equal(c1[0], B[12]["words"][3]) and list(counted) == [1]
        assert box.totals["not_a_ciphertext"] == 1 and box.totals["counted"] == 1


def test_box_k13_end_to_end(ctx):
    """the real shape, N = 1024 at k = 13 with the committed pinning: three proofs in, their sum out"""
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
    items = [(zk.Instances(b"".join(v.to_bytes(32, "little") for v in B[s]["inst"])), B[s]["proof"]) for s in (100, 101, 102)]
    with zk.BallotBox(ctx, vk, params, key[0], key[1]) as box:
        assert box.add(items) == [(zk.BALLOT_COUNTED, "")] * 3
        c0, c1, counted = box.tally()
        want0, want1, want_m = expect_tally(ctx, params, B, [(100, 0), (101, 0), (102, 0)], 1)
        assert np.array_equal(c0, want0) and np.array_equal(c1, want1) and list(counted) == [3]
        sk = np.array([int(x) % prm.Q for x in B[100]["sk"][::-1]], dtype=np.uint64)
        assert np.array_equal(ctx.bfv_decrypt(params, sk, c0[0], c1[0])[0], want_m[0])
        assert box.add(items[:1]) == [(zk.BALLOT_REPEATED, "")] and box.totals["counted"] == 3
