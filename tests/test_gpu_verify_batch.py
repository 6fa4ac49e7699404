"""Batch verification on the GPU (zkfhe_g1_decompress, zkfhe_msm_segmented, zkfhe_bfv_verify_batch): each kernel against the
oracle, and the batch verifier's verdict and reason for every proof against the single host verifier (zkfhe_bfv_verify).
Run on the MI355X box: pytest -m gpu."""
import json
import os
import random

import pytest

from oracle import binding as orc
from oracle import circuit_ref as C
from oracle import halo2_ref as H
from oracle import pyref
from oracle.point_encoding import point_compress, point_decompress

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "bfv")
Q, R = pyref.Q, pyref.R


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def chain(P, n):
    """P, 2P, ..., nP by repeated addition"""
    out, cur = [], None
    for _ in range(n):
        cur = pyref.g1_add(cur, P)
        out.append(cur)
    return out


def test_decompress_matches_oracle(ctx):
    rnd = random.Random(11)
    P = pyref.g1_mul(pyref.G1_GEN, rnd.randrange(1, R))
    pts = chain(P, 4095) + [None]
    enc = [point_compress(p) for p in pts]
    assert {p[1] & 1 for p in pts[:-1]} == {0, 1}
    q_bytes = bytearray(Q.to_bytes(32, "little"))
    big = bytearray((Q + 12345).to_bytes(32, "little"))
    x = 5
    while pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == 1:   # an x with no square root of x^3 + 3
        x += 1
    stray = bytearray(point_compress(None))
    stray[3] = 1
    signed_id = bytearray(point_compress(None))
    signed_id[31] |= 0x40
    enc += [bytes(q_bytes), bytes(big), x.to_bytes(32, "little"), bytes(stray), bytes(signed_id), b"\xff" * 32]
    got, st = ctx.g1_decompress(b"".join(enc))
    got_pts = orc.arr_to_points(got)
    for i, e in enumerate(enc):
        try:
            want = point_decompress(e)
        except AssertionError:
            assert st[i] != 0 and got_pts[i] is None, i
            continue
        assert st[i] == 0 and got_pts[i] == want, i
    assert list(st[-6:-1]) == [1, 1, 2, 3, 3]


def test_msm_segmented_matches_oracle(ctx):
    rnd = random.Random(12)
    base = chain(pyref.g1_mul(pyref.G1_GEN, rnd.randrange(1, R)), 96)
    pts = base + [None, pyref.g1_neg(base[3])]          # an identity point, and -P beside P
    ID, NEG3 = len(base), len(base) + 1
    segs = []
    for L in (0, 1, 2, 7, 700, 3000, 5):
        idx = [rnd.randrange(len(base)) for _ in range(L)]
        sc = [rnd.randrange(R) for _ in range(L)]
        if L == 7:
            idx[:4] = [3, NEG3, 3, ID]                    # P, -P, P repeated, the identity
            sc[:4] = [9, 9, R - 1, 5]
            sc[5] = 0
        if L == 5:
            idx, sc = [3, NEG3, 3, 3, 3], [R - 1, R - 1, 0, 1, 1]
        segs.append((idx, sc))
    index = [i for s in segs for i in s[0]]
    scal = [k for s in segs for k in s[1]]
    off = [0]
    for s in segs:
        off.append(off[-1] + len(s[0]))
    out = ctx.msm_segmented(orc.points_to_arr(pts), index, orc.ints_to_mont(scal).reshape(-1, 4), off)
    got = orc.arr_to_points(out)
    for j, (idx, sc) in enumerate(segs):
        if len(idx) > 100:
            want = orc.arr_to_points(orc.msm(orc.ints_to_mont(sc).reshape(1, -1, 4), orc.points_to_arr([pts[i] for i in idx])))[0]
        else:
            want = pyref.g1_msm(sc, [pts[i] for i in idx])
        assert got[j] == want, "segment %d (%d terms)" % (j, len(idx))
    import zk_fhe_amd as zk
    with pytest.raises(zk.ZkfheError):   # an index past the points
        ctx.msm_segmented(orc.points_to_arr(pts), [len(pts)], orc.ints_to_mont([1]).reshape(-1, 4), [0, 1])


# ---- proofs, made once per module ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def k13(ctx):
    """16 Poseidon proofs under three public keys and 4 Blake2b proofs, k = 13 (zk_fhe_amd.inputs: real BFV keygen + encrypt)"""
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    cfgj = json.load(open(os.path.join(G, "bfv_config.json")))
    prm = C.BfvParams()
    srs = zk.Srs(ctx, 13)
    out = {"srs_g2": srs.g2()}
    for kind, n in (("poseidon", 16), ("blake2b", 4)):
        pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), (1024, prm.Q, prm.T, prm.B),
                              zk.BfvConfig.from_pinning(cfgj, transcript=kind), replay=True)
        items = []
        for j in range(n):
            inp = inputs.generate(1024, prm.Q, prm.T, prm.B, seed=100 + j, key_seed=j % 3)
            proof, inst, _ = pk.prove(json.dumps(inp), b"batch-%d" % j)
            items.append((list(inst), proof))
        out[kind] = (pk.export_vk(), items)
        pk.destroy()
    srs.destroy()
    return out


def single(vk, items, **kw):
    import zk_fhe_amd as zk
    return [zk.bfv_verify(vk, inst, proof, **kw) for inst, proof in items]


def test_valid_batches(ctx, k13):
    import zk_fhe_amd as zk
    vk, items = k13["poseidon"]
    assert len({tuple(i[:8]) for i, _ in items}) == 3    # three public keys
    got = zk.bfv_verify_batch(ctx, vk, items)
    assert got == single(vk, items) == [(True, "")] * len(items)
    vkb, itb = k13["blake2b"]
    assert zk.bfv_verify_batch(ctx, vkb, itb) == single(vkb, itb) == [(True, "")] * len(itb)
    # one proof alone, and the external-G2 path
    assert zk.bfv_verify_batch(ctx, vk, items[:1]) == [(True, "")]
    g2, s_g2 = k13["srs_g2"]
    assert zk.bfv_verify_batch(ctx, vk, items[:5], g2=g2, s_g2=s_g2) == single(vk, items[:5], g2=g2, s_g2=s_g2) == [(True, "")] * 5
    # another SRS: every proof fails its pairing, batch and single alike
    assert zk.bfv_verify_batch(ctx, vk, items[:3], srs_seed=b"another-srs") == single(vk, items[:3], srs_seed=b"another-srs") == [(False, "")] * 3


def test_valid_batch_k14(ctx):
    import zk_fhe_amd as zk
    prm = C.BfvParams(N=16)
    from tests.test_proof_oracle import synth_input
    inps = [synth_input(16, prm.Q, prm.T, prm.B, s) for s in (5, 6)]
    hcfg = H.auto_config(14, 109, H.BfvCircuit(inps[0], prm))
    srs = zk.Srs(ctx, 14)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inps[0]), (16, prm.Q, prm.T, prm.B), zk.BfvConfig(14, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 109))
    items = []
    for j, inp in enumerate(inps):
        proof, inst, _ = pk.prove(json.dumps(inp), b"k14-%d" % j)
        items.append((list(inst), proof))
    vk = pk.export_vk()
    pk.destroy()
    srs.destroy()
    assert zk.bfv_verify_batch(ctx, vk, items) == single(vk, items) == [(True, "")] * 2


def recompress(proof, word, P):
    b = bytearray(proof)
    b[32 * word:32 * word + 32] = point_compress(P)
    return bytes(b)


def test_tamper_matrix(ctx, k13):
    import zk_fhe_amd as zk
    vk, items = k13["poseidon"]
    good = items[:6]
    inst, proof = items[6]
    flip = bytearray(proof)
    flip[len(proof) - 100] ^= 1                               # an evaluation (scalar) byte
    inst2 = list(inst)
    inst2[-1] = (inst2[-1] + 1) % R                            # a public input
    swap = bytearray(proof)
    swap[0:32], swap[32:64] = proof[32:64], proof[0:32]        # two commitments swapped
    big = bytearray(proof)
    big[32:64] = (Q + 7).to_bytes(32, "little")                # x >= q
    x = 5
    while pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == 1:
        x += 1
    off = bytearray(proof)
    off[64:96] = x.to_bytes(32, "little")                      # an x off the curve
    bad = [
        (inst, bytes(flip)), (inst2, proof), (inst, bytes(swap)), (inst, proof[:-32]), (inst, proof + b"\0"),
        (inst, bytes(big)), (inst, bytes(off)), (inst, recompress(proof, 2, None)),   # the identity: Poseidon refuses it
        (inst + [0] * 8192, proof),                           # more instances than usable rows
    ]
    mixed = []
    for j in range(max(len(good), len(bad))):
        if j < len(good):
            mixed.append(good[j])
        if j < len(bad):
            mixed.append(bad[j])
    got = zk.bfv_verify_batch(ctx, vk, mixed)
    want = single(vk, mixed)
    assert got == want
    assert sum(ok for ok, _ in got) == len(good)
    assert sum(1 for _, why in got if why) >= 6     # decoding / transcript rejections carry their reason


@pytest.fixture(scope="module")
def toy3():
    """Three oracle-made toy proofs (k = 9, 278 words) under one proving key: A and B of one public key, C of a second one
    (the proving key does not depend on the public key: the oracle prover takes either circuit)."""
    import zk_fhe_amd as zk
    prm = C.BfvParams(N=8)
    from tests.test_proof_oracle import synth_input
    inp = synth_input(8, prm.Q, prm.T, prm.B, 1)
    circ = H.BfvCircuit(inp, prm)
    cfg = H.auto_config(9, 9, circ)
    srs = H.make_srs(9)
    pk, _ = H.keygen_circuit(cfg, circ, srs)
    vkb = zk.make_vk_bytes(cfg.k, cfg.n_gate0, cfg.n_gate1, cfg.n_lookup, cfg.n_rlc, cfg.unusable_rows, cfg.lookup_bits,
                           pk.vk_digest, pk.fixed_commit, pk.sigma_commit, "poseidon")
    circ2 = H.BfvCircuit(synth_input(8, prm.Q, prm.T, prm.B, 2), prm)
    proofs = [H.prove(cfg, pk, srs, c, seed) for c, seed in ((circ, b"A"), (circ, b"B"), (circ2, b"C"))]
    assert proofs[0][1][:16] == proofs[1][1][:16] != proofs[2][1][:16]      # pk0 | pk1: two prefix groups
    return pk, srs, vkb, proofs


def test_randomisers_defeat_cancellation(ctx, toy3):
    """Two valid toy proofs A, B with h2 moved by D, D' so that the UNWEIGHTED sum of their pairing equations still holds: the
    randomised batch must reject exactly A and B."""
    import zk_fhe_amd as zk
    pk, srs, vkb, proofs = toy3
    # uu of each proof: the last challenge of the oracle verifier's replay
    T = H.TRANSCRIPTS["poseidon"]
    orig = T.squeeze
    seen = []

    def rec(self):
        v = orig(self)
        seen.append(v)
        return v
    T.squeeze = rec
    try:
        uus = []
        for proof, inst in proofs[:2]:
            seen.clear()
            assert H.verify(H.VerifyingKey(pk), srs, inst, proof)
            uus.append(seen[-1])
    finally:
        T.squeeze = orig
    s = srs["s"]
    n_words = len(proofs[0][0]) // 32
    W = [point_decompress(p[0][32 * (n_words - 1):]) for p in proofs[:2]]
    D = pyref.g1_mul(pyref.G1_GEN, (uus[1] - s) % R)
    D2 = pyref.g1_mul(pyref.G1_GEN, (-(uus[0] - s)) % R)
    # (uu_A - s) D + (uu_B - s) D' = 0 in G1: the unweighted sum of the two equations cancels
    assert pyref.g1_add(pyref.g1_mul(D, (uus[0] - s) % R), pyref.g1_mul(D2, (uus[1] - s) % R)) is None
    A = recompress(proofs[0][0], n_words - 1, pyref.g1_add(W[0], D))
    B = recompress(proofs[1][0], n_words - 1, pyref.g1_add(W[1], D2))
    items = [(proofs[2][1], proofs[2][0]), (proofs[0][1], A), (proofs[1][1], B), (proofs[0][1], proofs[0][0])]
    got = zk.bfv_verify_batch(ctx, vkb, items)
    assert got == single(vkb, items) == [(True, ""), (False, ""), (False, ""), (True, "")]


# ---- across the chunk boundary: 260 toy proofs, 256 per device pass -----------------------------------------------------------

N_CHUNKED = 260


@pytest.fixture(scope="module")
def single_memo():
    """the single verifier's (verdict, reason), computed once per distinct (instances, proof)"""
    import zk_fhe_amd as zk
    memo = {}

    def want(vkb, items):
        out = []
        for inst, proof in items:
            key = (tuple(inst), proof)
            if key not in memo:
                memo[key] = zk.bfv_verify(vkb, inst, proof)
            out.append(memo[key])
        return out
    return want


def cycled(proofs):
    """260 good items: the three toy proofs in turn, so both public-key groups have members on either side of item 256"""
    return [(list(proofs[j % 3][1]), proofs[j % 3][0]) for j in range(N_CHUNKED)]


def test_two_chunks_all_good(ctx, toy3, single_memo):
    import zk_fhe_amd as zk
    _, _, vkb, proofs = toy3
    items = cycled(proofs)
    got = zk.bfv_verify_batch(ctx, vkb, items)
    assert got == single_memo(vkb, items) == [(True, "")] * N_CHUNKED


def test_two_chunks_bad_items_around_the_boundary(ctx, toy3, single_memo):
    """Bad items at 254, 255 (end of the first pass) and 256, 257, 259 (start of the second): the batch pairing fails, so every
    other item is accepted by its own pairing; every verdict and reason is the single verifier's."""
    import zk_fhe_amd as zk
    _, _, vkb, proofs = toy3
    items = cycled(proofs)
    x = 5
    while pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == 1:   # an x with no square root of x^3 + 3
        x += 1

    def tamper(j, f_inst=lambda i: i, f_proof=lambda p: p):
        inst, proof = items[j]
        items[j] = (f_inst(list(inst)), f_proof(proof))

    def flip(p):
        b = bytearray(p)
        b[len(p) - 100] ^= 1                                         # an evaluation (scalar) byte
        return bytes(b)
    tamper(254, f_proof=flip)
    tamper(255, f_proof=lambda p: p[:-32])                           # one word short
    tamper(256, f_proof=lambda p: p[:64] + x.to_bytes(32, "little") + p[96:])   # an x off the curve in commitment 2
    tamper(257, f_proof=lambda p: recompress(p, 2, None))            # the identity in commitment 2: Poseidon refuses it
    tamper(259, f_inst=lambda i: i[:-1] + [(i[-1] + 1) % R])         # a public input off by one
    bad = {254, 255, 256, 257, 259}
    got = zk.bfv_verify_batch(ctx, vkb, items)
    assert got == single_memo(vkb, items)
    assert [j for j, (ok, _) in enumerate(got) if not ok] == sorted(bad)
    assert got[254] == (False, "") and got[259] == (False, "") and got[255] == (False, "proof truncated")
    assert got[256] == (False, "point not on curve") and got[257][1] != ""


def test_first_chunk_all_rejected_before_the_pairing(ctx, toy3, single_memo):
    """The whole first device pass leaves no segment (every proof is one word short), the second pass is live."""
    import zk_fhe_amd as zk
    _, _, vkb, proofs = toy3
    items = [(inst, proof[:-32] if j < 256 else proof) for j, (inst, proof) in enumerate(cycled(proofs))]
    got = zk.bfv_verify_batch(ctx, vkb, items)
    assert got == single_memo(vkb, items) == [(False, "proof truncated")] * 256 + [(True, "")] * 4


def test_arguments(ctx, k13):
    import ctypes
    import zk_fhe_amd as zk
    vk, items = k13["poseidon"]
    with pytest.raises(zk.ZkfheError):
        zk.bfv_verify_batch(ctx, vk, [])
    lib = zk.load_library()
    ok = (ctypes.c_int * 1)()
    assert lib.zkfhe_bfv_verify_batch(None, vk, len(vk), 1, None, None, None, None, None, 0, None, None, ok, None, 0) == zk_einval()
    assert lib.zkfhe_bfv_verify_batch(ctx.h, vk, len(vk), 1, None, None, None, None, None, 0, None, None, ok, None, 0) == zk_einval()
    # a corrupt vk rejects every proof with the single verifier's reason
    vk2 = bytearray(vk)
    vk2[100] ^= 1
    got = zk.bfv_verify_batch(ctx, bytes(vk2), items[:3])
    assert got == single(bytes(vk2), items[:3]) and all(not ok and "digest" in why for ok, why in got)


def zk_einval():
    return -1
