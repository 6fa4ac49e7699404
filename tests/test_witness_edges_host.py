"""The witness generator at the edges of its values, on moduli of 29, 32, 33, 60 and 63 bits -- the host half: inputs crafted so that
the range gadgets meet their boundaries (a = z, z + 1, y - z - 1, y - z: `shifted` all 0xff bytes, or all zero bytes under a top limb
of 1), div_mod meets remainder 0 and Q - 1, quotient 0 and its largest dividend N (Q - 1)^2 (a quotient above 64 bits with the 63-bit
Q), a 32-bit Q puts the gadgets' limbs on a word boundary, and the polynomials degenerate (u = 0, u = x).  Every input is an honest
encryption, so the oracle restatement (oracle/circuit_ref.py) accepts it; the library's tables must equal the oracle's, cell for cell,
on both phase-0 paths.  tests/test_gpu_witness_edges.py runs the same inputs through the device generator and the prover.
CPU only: zkfhe_bfv_build_tables does not touch the GPU (wide products then come from the restatement on both paths)."""
import functools
import json
import random

import numpy as np
import pytest

import zk_fhe_amd as zk
from oracle import binding as orc
from oracle import circuit_ref as C
from oracle import halo2_ref as H
from tests.test_proof_oracle import craft, negacyclic

N, K, UNUSABLE = 256, 12, 109   # gadget launches of 256, 257, 511 and 513 threads: on both sides of a workgroup
GAMMA = 0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA987654321 % H.R
SETS = {   # name: (Q, T, B)
    "Q29": (536870909, 7, 19),
    "Q32": ((1 << 32) - 5, 7, 19),           # c_pow2(32), c_low, c_byte exactly on a limb boundary; still gl::poly_mul_u32
    "Q33": ((1 << 32) + 15, 7, 19),          # the first width that takes the convolution backend in a proof
    "Q60": ((1 << 60) - 93, 65537, 19),
    "Q63": ((1 << 63) - 25, 7, 19),          # the divider's bound q < 2^63; quotients of 71 bits
}
INPUTS = ("max", "max_mixed", "zero_u", "residues", "range_walk")
# residues: (m_i, e0_i, target) as functions of (Q, T, B): pk0 is chosen so that pu0_i + delta m_i + e0_i = target (mod Q)
TRIPLES = [lambda Q, T, B: (0, 0, 0), lambda Q, T, B: (0, 0, Q - 1), lambda Q, T, B: (T // 2, B, 0), lambda Q, T, B: (T // 2, B, Q - 1),
           lambda Q, T, B: (Q - T // 2, Q - B, 0), lambda Q, T, B: (Q - 1, Q - 1, Q - 1), lambda Q, T, B: (1, Q - B, 0),
           lambda Q, T, B: (Q - T // 2, B, 1)]
# ... and (e1_i, pu1_i) for c1
PAIRS = [lambda Q, B: (0, 0), lambda Q, B: (Q - 1, Q - 1), lambda Q, B: (1, Q - 1), lambda Q, B: (B, Q - B), lambda Q, B: (Q - B, B),
         lambda Q, B: (Q - 1, 0), lambda Q, B: (B, 0), lambda Q, B: (Q - B, 0)]


def allowed(Q, z):
    """[0, z] u [Q - z, Q - 1], the set constrain_coefficients_in_range admits"""
    return list(range(0, z + 1)) + list(range(Q - z, Q))


def walk(Q, z, n, stride=1, start=0):
    """n values cycling through every element of allowed(Q, z); a set longer than n (m under T = 65537) gives its four ends instead:
    up from 0, up to z, up from Q - z, up to Q - 1, a quarter of n each"""
    if 2 * z + 1 <= n:
        s = allowed(Q, z)
        return [s[(start + stride * i) % len(s)] for i in range(n)]
    q = n // 4
    s = list(range(0, q)) + list(range(z - q + 1, z + 1)) + list(range(Q - z, Q - z + q)) + list(range(Q - (n - 3 * q), Q))
    return [s[(start + stride * i) % n] for i in range(n)]


def residue_slots(n):
    """where the eight triples sit: the first indices, the middle, and the last indices up to n - 2 (u = x ties index n - 1 to pk[0])"""
    assert n >= 32
    return list(range(8)) + list(range(n // 2 - 4, n // 2 + 4)) + list(range(n - 9, n - 1))


def residue_sums(inp, Q, T):
    """the dividends of the two closing div_mod calls as Python integers: pu0 + delta m + e0 and pu1 + e1 with u = x"""
    pk0, pk1, m, e0, e1 = ([int(x) for x in inp[k]] for k in ("pk0", "pk1", "m", "e0", "e1"))
    n = len(pk0)
    pu0 = pk0[1:] + [Q - pk0[0]]
    pu1 = pk1[1:] + [Q - pk1[0]]
    return [pu0[i] + (Q // T) * m[i] + e0[i] for i in range(n)], [pu1[i] + e1[i] for i in range(n)], pu0, pu1


def crafted(name, n, Q, T, B):
    """the crafted input `name` as an input dict (tests/test_proof_oracle.py::craft computes c0 and c1)"""
    z = T // 2
    if name == "max":
        return craft(n, Q, T, [Q - 1] * n, [Q - 1] * n, [Q - 1] * n, [z] * n, [B] * n, [Q - B] * n)
    if name == "max_mixed":
        return craft(n, Q, T, [Q - 1] * n, [Q - 1] * n, [1] * n, [Q - z] * n, [Q - B] * n, [B] * n)
    if name == "zero_u":
        return craft(n, Q, T, [Q - 1] * n, [1] * n, [0] * n, [0] * n, [0] * n, [0] * n)
    if name == "degree0_u":   # not a parity case: the reference panics on the empty quotient, the library must refuse
        rng = random.Random(40)
        return craft(n, Q, T, [rng.randrange(1, Q) for _ in range(n)], [rng.randrange(1, Q) for _ in range(n)], [0] * (n - 1) + [1], [0] * n, [0] * n, [0] * n)
    rng = random.Random(41 if name == "residues" else 42)
    pk0 = [rng.randrange(1, Q) for _ in range(n)]
    pk1 = [rng.randrange(1, Q) for _ in range(n)]
    if name == "residues":
        m = [rng.choice(allowed(Q, min(z, 3))) for _ in range(n)]
        e0 = [rng.choice(allowed(Q, B)) for _ in range(n)]
        e1 = [rng.choice(allowed(Q, B)) for _ in range(n)]
        delta = Q // T
        for k, i in enumerate(residue_slots(n)):
            m[i], e0[i], target = TRIPLES[k % 8](Q, T, B)
            pk0[i + 1] = (target - delta * m[i] - e0[i]) % Q
            e1[i], pk1[i + 1] = PAIRS[k % 8](Q, B)
        assert pk0[0] and pk1[0]   # slots start at pk[1]: the quotient's leading coefficient stays non-zero
        return craft(n, Q, T, pk0, pk1, [0] * (n - 2) + [1, 0], m, e0, e1)
    assert name == "range_walk"
    return craft(n, Q, T, pk0, pk1, [(0, 1, Q - 1)[i % 3] for i in range(n)], walk(Q, z, n), walk(Q, B, n), walk(Q, B, n, stride=7, start=3))


def assert_edges(name, inp, Q, T, B):
    """the input holds what its name says -- from Python integers, before anything is compared"""
    v = {k: [int(x) for x in inp[k]] for k in ("pk0", "pk1", "m", "u", "e0", "e1", "c0", "c1")}
    n, z = len(v["u"]), T // 2
    if name in ("max", "max_mixed"):
        assert set(v["pk0"]) == set(v["pk1"]) == {Q - 1}
        if name == "max":
            # the middle coefficient of the plain product pk0 * u: the largest dividend div_mod ever sees
            assert sum(v["pk0"][i] * v["u"][n - 1 - i] for i in range(n)) == n * (Q - 1) ** 2
            assert n * (Q - 1) ** 2 < 1 << 192 and (Q.bit_length() < 63 or n * (Q - 1) ** 2 // Q >= 1 << 64)   # the divider's third word
            assert (set(v["m"]), set(v["e0"]), set(v["e1"])) == ({z}, {B}, {Q - B})
        else:
            assert (set(v["u"]), set(v["m"]), set(v["e0"]), set(v["e1"])) == ({1}, {Q - z}, {Q - B}, {B})
    elif name == "zero_u":
        assert not any(v["u"]) and not any(v["c0"]) and not any(v["c1"]) and set(v["pk0"]) == {Q - 1} and set(v["pk1"]) == {1}
    elif name == "residues":
        assert v["u"] == [0] * (n - 2) + [1, 0]
        s0, s1, pu0, pu1 = residue_sums(inp, Q, T)
        assert negacyclic(v["pk0"], v["u"], n, Q) == pu0 and negacyclic(v["pk1"], v["u"], n, Q) == pu1
        assert pu0[:n - 1] == v["pk0"][1:] and pu0[n - 1] == Q - v["pk0"][0] and v["pk0"][0] and v["pk1"][0]
        assert v["c0"] == [s % Q for s in s0] and v["c1"] == [s % Q for s in s1]
        sums = s0 + s1
        assert any(s % Q == 0 and s // Q >= 1 for s in sums), "remainder 0 under a quotient >= 1"
        assert any(s % Q == Q - 1 for s in sums), "remainder Q - 1"
        assert 0 in sums, "the value 0"
        assert {0, 1, 2} <= {s // Q for s in sums}, "quotients 0, 1 and 2"
        for k, i in enumerate(residue_slots(n)):   # every triple landed, in all three blocks
            assert (v["m"][i], v["e0"][i], s0[i] % Q) == TRIPLES[k % 8](Q, T, B) and (v["e1"][i], pu1[i]) == PAIRS[k % 8](Q, B)
        assert n - 2 in residue_slots(n) and 0 in residue_slots(n)
    elif name == "range_walk":
        for key, bound in (("e0", B), ("e1", B), ("m", z)):
            have = set(v[key])
            assert have <= set(allowed(Q, bound)) if 2 * bound + 1 <= n else all(x <= bound or x >= Q - bound for x in have)
            assert {0, 1, bound - 1, bound, Q - bound, Q - bound + 1, Q - 1} <= have, key   # a = z, and a = y - z, from inside
            if 2 * bound + 1 <= n:
                assert have == set(allowed(Q, bound)), key
        assert set(v["u"]) == {0, 1, Q - 1}
    elif name == "degree0_u":
        assert v["u"] == [0] * (n - 1) + [1] and all(v["pk0"]) and all(v["pk1"])
    else:
        raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def column_counts(set_name):
    """(n_gate0, n_gate1, n_lookup, n_rlc) at 2^K rows: the layout depends on the parameters only, so one probe with room to spare
    gives the break points of every input of the set.  All five sets fit K = 12."""
    Q, T, B = SETS[set_name]
    text = json.dumps(crafted("zero_u", N, Q, T, B))
    probe = zk.bfv_build_tables(text, (N, Q, T, B), zk.BfvConfig(K, 8, 480, 160, 16, UNUSABLE), 1, keygen_mode=False)
    n0, n1, nr = (len(probe["break_points"][w]) + 1 for w in ("gate0", "gate1", "rlc"))
    nl = -(-probe["lookups"] // ((1 << K) - UNUSABLE))
    assert n0 < 8 and n1 < 480 and nl < 160 and nr < 16
    return n0, n1, nl, nr


def oracle_contexts(inp, prm, gamma=GAMMA):
    ctx0, pub, st = C.bfv_phase0(inp, prm)
    ctx_gate, ctx_rlc = C.bfv_phase1(st, prm, gamma)
    return ctx0, pub, ctx_gate, ctx_rlc


def violations(ctx0, ctx_gate, ctx_rlc, gamma=GAMMA):
    """the gates, copies, constants and lookups of tests/test_witness_oracle.py::test_gates_hold, counted instead of asserted"""
    R = C.R
    bad = []
    for ctx in (ctx0, ctx_gate):
        a = ctx.advice
        bad += [("gate", ctx.cid, o) for o in ctx.selector if (a[o] + a[o + 1] * a[o + 2] - a[o + 3]) % R]
    a = ctx_rlc.advice
    bad += [("rlc", ctx_rlc.cid, o) for o in ctx_rlc.selector if (a[o] * gamma + a[o + 1] - a[o + 2]) % R]
    vals = {ctx.cid: ctx.advice for ctx in (ctx0, ctx_gate, ctx_rlc)}
    for ctx in (ctx0, ctx_gate, ctx_rlc):
        bad += [("copy", c1, o1) for (c1, o1), (c2, o2) in ctx.copies if vals[c1][o1] != vals[c2][o2]]
        bad += [("const", c1, o1) for (c1, o1), v in ctx.consts if vals[c1][o1] != v]
        bad += [("lookup", c1, o1) for (c1, o1) in ctx.lookup if not 0 <= vals[c1][o1] < 256]
    return bad


def ints(arr):
    return orc.arr_to_ints(np.ascontiguousarray(arr).reshape(-1, 4))


def tables(text, prm, zcfg, mode, monkeypatch):
    if mode == "generic":
        monkeypatch.setenv("ZKFHE_PHASE0", "generic")
    else:
        monkeypatch.delenv("ZKFHE_PHASE0", raising=False)
    return zk.bfv_build_tables(text, prm, zcfg, GAMMA, keygen_mode=False)


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("set_name", sorted(SETS))
def test_tables_match_the_oracle_on_crafted_inputs(set_name, name, monkeypatch):
    """advice table and instance of zkfhe_bfv_build_tables against H.assign of bfv_phase0 / bfv_phase1, on the machine-word phase 0 and
    on the restatement (ZKFHE_PHASE0=generic): the oracle's cells satisfy every constraint, and both paths give its bytes"""
    Q, T, B = SETS[set_name]
    inp = crafted(name, N, Q, T, B)
    assert_edges(name, inp, Q, T, B)
    n0, n1, nl, nr = column_counts(set_name)
    ctx0, pub, ctx_gate, ctx_rlc = oracle_contexts(inp, C.BfvParams(N=N, Q=Q, T=T, B=B))
    assert violations(ctx0, ctx_gate, ctx_rlc) == []
    A = H.assign(H.Config(K, n0, n1, nl, nr, UNUSABLE), ctx0, ctx_gate, ctx_rlc, pub)
    want_adv = [v for col in A.advice for v in col]
    text = json.dumps(inp)
    seen = []
    for mode in ("fast", "generic"):
        t = tables(text, (N, Q, T, B), zk.BfvConfig(K, n0, n1, nl, nr, UNUSABLE), mode, monkeypatch)
        assert t["cells"] == (len(ctx0.advice), len(ctx_gate.advice), len(ctx_rlc.advice)) and t["lookups"] == len(ctx_gate.lookup)
        assert ints(t["instance"]) == A.instance, mode
        got_adv = ints(t["advice"])
        assert len(got_adv) == len(want_adv)
        diff = next((i for i, (a, b) in enumerate(zip(got_adv, want_adv)) if a != b), None)
        assert diff is None, "%s: first differing advice cell: column %d row %d" % (mode, diff // (1 << K), diff % (1 << K))
        seen.append((t["advice"].tobytes(), t["instance"].tobytes()))
    assert seen[0] == seen[1]


@pytest.mark.parametrize("set_name", sorted(SETS))
def test_degree_zero_u_is_refused_on_both_phase0_paths(set_name, monkeypatch):
    """u = 1: the quotient of pk_i u by x^N + 1 is empty and the reference panics (src/poly.rs:158).  The Python oracle pads it with
    zeros instead -- a known divergence, so there is nothing to compare with; the library refuses, with the same words on either
    path, and builds the next valid input as before."""
    Q, T, B = SETS[set_name]
    bad = crafted("degree0_u", N, Q, T, B)
    assert_edges("degree0_u", bad, Q, T, B)
    n0, n1, nl, nr = column_counts(set_name)
    zcfg = zk.BfvConfig(K, n0, n1, nl, nr, UNUSABLE)
    good = json.dumps(crafted("zero_u", N, Q, T, B))
    before = tables(good, (N, Q, T, B), zcfg, "fast", monkeypatch)["advice"].tobytes()
    said = []
    for mode in ("fast", "generic"):
        with pytest.raises(zk.ZkfheError) as e:
            tables(json.dumps(bad), (N, Q, T, B), zcfg, mode, monkeypatch)
        said.append(str(e.value))
        assert tables(good, (N, Q, T, B), zcfg, mode, monkeypatch)["advice"].tobytes() == before
    assert said[0] == said[1] and "quotient" in said[0]
