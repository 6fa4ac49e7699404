"""The device witness generator (k_gadget of zk-fhe_amd/host/gpu_witness.hip.hpp: one thread per coefficient) and the prover on the
crafted inputs of tests/test_witness_edges_host.py: range gadgets at a = z, z + 1, y - z - 1, y - z, div_mod at remainder 0 and Q - 1,
quotient 0 and the largest dividend, moduli of 29, 32, 33, 60 and 63 bits (a limb boundary; both sides of the switch from the host
product to the convolution backend; the divider's bound), u = 0 and u = x -- cell for cell against the oracle, proofs against the
verifier, the host generator and the oracle prover, and every one-cell step off an edge refused.
Run on the MI355X box:  python -m pytest tests/test_gpu_witness_edges.py -m gpu -q"""
import json
import os

import numpy as np
import pytest

from oracle import circuit_ref as C
from tests.test_witness_edges_host import (GAMMA, INPUTS, K, N, SETS, UNUSABLE, assert_edges, column_counts, crafted, oracle_contexts,
                                           violations)

pytestmark = pytest.mark.gpu
MASK = (1 << 64) - 1
# one coefficient changed, nothing recomputed: (field, new value as a function of (Q, T, B, old value))
STEPS = {
    "e0=B+1": ("e0", lambda Q, T, B, old: B + 1), "e0=Q-B-1": ("e0", lambda Q, T, B, old: Q - B - 1),
    "e1=B+1": ("e1", lambda Q, T, B, old: B + 1), "e1=Q-B-1": ("e1", lambda Q, T, B, old: Q - B - 1),
    "m=T//2+1": ("m", lambda Q, T, B, old: T // 2 + 1), "m=Q-T//2-1": ("m", lambda Q, T, B, old: Q - T // 2 - 1),
    "u=2": ("u", lambda Q, T, B, old: 2), "u=Q-2": ("u", lambda Q, T, B, old: Q - 2),
    "c0+1": ("c0", lambda Q, T, B, old: (old + 1) % Q), "c0-1": ("c0", lambda Q, T, B, old: (old - 1) % Q),
    "c1+1": ("c1", lambda Q, T, B, old: (old + 1) % Q), "c1-1": ("c1", lambda Q, T, B, old: (old - 1) % Q),
}


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx):
    """one proving key per parameter set, all in 2^12 rows on one SRS (every set fits K = 12)"""
    import zk_fhe_amd as zk
    srs = zk.Srs(ctx, K)
    pks = {}
    for name, (Q, T, B) in SETS.items():
        n0, n1, nl, nr = column_counts(name)
        pks[name] = zk.BfvProvingKey(ctx, srs, json.dumps(crafted("zero_u", N, Q, T, B)), (N, Q, T, B), zk.BfvConfig(K, n0, n1, nl, nr, UNUSABLE))
    yield pks
    for pk in pks.values():
        pk.destroy()
    srs.destroy()


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("set_name", sorted(SETS))
def test_device_stream_equals_the_oracle_cell_for_cell(keys, set_name, name):
    """the phase-1 gate cells of the gadget kernels against bfv_phase1 of the oracle; a mismatch names its gadget call, coefficient and offset"""
    Q, T, B = SETS[set_name]
    inp = crafted(name, N, Q, T, B)
    assert_edges(name, inp, Q, T, B)
    want = oracle_contexts(inp, C.BfvParams(N=N, Q=Q, T=T, B=B))[2].advice
    got = keys[set_name].witness_stream(json.dumps(inp), GAMMA)
    ref = np.array([[(v >> (64 * j)) & MASK for j in range(4)] for v in want], dtype=np.uint64)
    assert got.shape == ref.shape
    bad = np.nonzero((got != ref).any(axis=1))[0]
    if bad.size:
        first = int(bad[0])
        raise AssertionError("first differing cell: %d of %d (%s); %d cells differ" % (first, len(want), locate(gadget_calls(inp, Q, T, B), first), bad.size))


def gadget_calls(inp, Q, T, B):
    """[(PolyChip method, first cell, cells, coefficients)] of the phase-1 gate stream, recorded from the oracle as it runs"""
    from unittest import mock
    calls = []

    def traced(name):
        inner = getattr(C.PolyChip, name)

        def run(self, *args, **kw):
            gate = next(a for a in args if isinstance(a, C.Context) and not a.rlc)
            start = len(gate.advice)
            out = inner(self, *args, **kw)
            calls.append((name, start, len(gate.advice) - start, self.degree + 1 if name != "constrain_mul" else 1))
            return out
        return mock.patch.object(C.PolyChip, name, run)
    names = ("constrain_coefficients_in_range", "constrain_from_distribution_chi_key", "constrain_mul", "reduce_by_modulo",
             "constrain_coefficients_in_modulus_field", "add", "scalar_mul", "constrain_equality")
    patches = [traced(n) for n in names]
    for p in patches:
        p.start()
    try:
        total = len(oracle_contexts(inp, C.BfvParams(N=N, Q=Q, T=T, B=B))[2].advice)
    finally:
        for p in patches:
            p.stop()
    assert sum(c[2] for c in calls) == total and all(c[2] % c[3] == 0 for c in calls)
    return calls


def locate(calls, cell):
    """the gadget call a stream cell belongs to, its coefficient, and the offset inside that coefficient's block"""
    for j, (name, start, size, count) in enumerate(calls):
        if start <= cell < start + size:
            per = size // count
            return "call %d, %s: coefficient %d, offset %d of %d" % (j, name, (cell - start) // per, (cell - start) % per, per)
    return "outside every gadget call"


@pytest.mark.parametrize("name", ["max", "residues"])
@pytest.mark.parametrize("set_name", sorted(SETS))
def test_proofs_verify_and_do_not_depend_on_the_witness_path(keys, set_name, name):
    """the proof is accepted, and the host generator (ZKFHE_WITNESS=host) and the plain commitment order (ZKFHE_EARLY_P1=0) give its bytes"""
    import zk_fhe_amd as zk
    Q, T, B = SETS[set_name]
    inp = crafted(name, N, Q, T, B)
    assert_edges(name, inp, Q, T, B)
    text, pk, seed = json.dumps(inp), keys[set_name], ("edge-%s-%s" % (set_name, name)).encode()
    try:
        os.environ.pop("ZKFHE_WITNESS", None)
        os.environ.pop("ZKFHE_EARLY_P1", None)
        dev, inst, _ = pk.prove(text, seed)
        ok, why = zk.bfv_verify(pk.export_vk(), inst, dev)
        assert ok, why
        pub = [int(x) for k in ("pk0", "pk1", "c0", "c1", "cyclo") for x in inp[k]]
        assert inst == pub
        os.environ["ZKFHE_WITNESS"] = "host"
        host, inst_h, _ = pk.prove(text, seed)
        assert inst_h == inst and host == dev
        os.environ.pop("ZKFHE_WITNESS", None)
        os.environ["ZKFHE_EARLY_P1"] = "0"
        plain, inst_p, _ = pk.prove(text, seed)
        assert inst_p == inst and plain == dev
    finally:
        os.environ.pop("ZKFHE_WITNESS", None)
        os.environ.pop("ZKFHE_EARLY_P1", None)


@pytest.mark.parametrize("name", ["max", "zero_u"])
def test_toy_proofs_of_degenerate_columns_match_the_oracle_prover(ctx, name):
    """N = 8 in 2^9 rows with the 29-bit Q: constant columns, all-zero columns and lookup bytes of 0x00 / 0xff only through the grand
    products and the lookup argument, byte for byte.  The oracle prover's Python is most of the 15 s or so a case takes."""
    from tests.test_gpu_fr9_kernels import prove_and_compare
    Q, T, B = SETS["Q29"]
    assert (Q, T, B) == (C.BfvParams().Q, C.BfvParams().T, C.BfvParams().B)
    inp = crafted(name, 8, Q, T, B)
    assert_edges(name, inp, Q, T, B)
    prove_and_compare(ctx, 8, 9, 9, inp, b"edge-" + name.encode())


@pytest.mark.parametrize("where", ["first", "interior", "last"])
@pytest.mark.parametrize("step", sorted(STEPS))
@pytest.mark.parametrize("set_name", ["Q29", "Q63"])
def test_one_cell_off_an_edge_is_refused(keys, set_name, step, where):
    """range_walk with one coefficient moved one step out of its set (or one ciphertext coefficient off by one) and nothing recomputed:
    the oracle's own gates, copies, constants and lookups name a violated constraint first, then the prover answers with a status --
    and proves the unmodified input to the same bytes before and after.  An ordinary invalid witness: nothing here faults anything."""
    import zk_fhe_amd as zk
    Q, T, B = SETS[set_name]
    good = crafted("range_walk", N, Q, T, B)
    assert_edges("range_walk", good, Q, T, B)
    pk, prm = keys[set_name], C.BfvParams(N=N, Q=Q, T=T, B=B)
    field, new = STEPS[step]
    i = {"first": 0, "interior": 101, "last": N - 1}[where]
    bad = dict(good)
    vals = list(good[field])
    vals[i] = str(new(Q, T, B, int(vals[i])))
    assert vals[i] != good[field][i] and 0 <= int(vals[i]) < Q
    bad[field] = vals
    assert sum(a != b for k in good for a, b in zip(good[k], bad[k])) == 1
    ctx0, _, ctx_gate, ctx_rlc = oracle_contexts(bad, prm)
    assert violations(ctx0, ctx_gate, ctx_rlc), "the altered input satisfies the circuit: nothing to refuse"
    before = pk.prove(json.dumps(good), b"edge-walk")[0]
    with pytest.raises(zk.ZkfheError):
        pk.prove(json.dumps(bad), b"edge-walk")
    assert pk.prove(json.dumps(good), b"edge-walk")[0] == before


@pytest.mark.parametrize("set_name", sorted(SETS))
def test_degree_zero_u_is_refused_with_a_status(keys, set_name):
    """u = 1 leaves an empty quotient, on which the reference panics: prove and witness_stream refuse it, and the key still works"""
    import zk_fhe_amd as zk
    Q, T, B = SETS[set_name]
    bad = crafted("degree0_u", N, Q, T, B)
    assert_edges("degree0_u", bad, Q, T, B)
    good = json.dumps(crafted("zero_u", N, Q, T, B))
    pk = keys[set_name]
    before = pk.prove(good, b"edge-deg0")[0]
    stream = pk.witness_stream(good, GAMMA)
    with pytest.raises(zk.ZkfheError):
        pk.prove(json.dumps(bad), b"edge-deg0")
    with pytest.raises(zk.ZkfheError):
        pk.witness_stream(json.dumps(bad), GAMMA)
    assert pk.prove(good, b"edge-deg0")[0] == before
    assert np.array_equal(pk.witness_stream(good, GAMMA), stream)
