"""The throughput profile of a proof (zkfhe_prover_gate(n > 0), or ZKFHE_PROFILE=throughput): more elements per inversion in the long
batch inversions, chunks of 256 points in the table sums of a few columns, no early phase-1 commitment -- scheduling only.  The proof
bytes under either profile are the oracle's, the override wins over the gate either way, and a k = 13 proof under the gate is the
59-launch chain without the early commitment.  Run on the MI355X box: pytest -m gpu."""
import json
import os

import pytest

from oracle import circuit_ref as C
from oracle import halo2_ref as H
from tests.test_gpu_prover import first_diff, oracle_k13
from tests.test_proof_oracle import synth_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("transcript", ["poseidon", "blake2b"])
def test_toy_proof_bytes_do_not_depend_on_the_profile(ctx, monkeypatch, transcript):
    """Toy circuit (N = 8 ring, k = 9): gate 0 and gate 4, then ZKFHE_PROFILE set each way with the gate at the opposite value: four
    times the oracle's bytes.  That the profile really switched shows in the launch count: with the Poseidon transcript the throughput
    profile leaves out the early phase-1 commitment, and the override decides it against the gate."""
    import zk_fhe_amd as zk
    for v in ("ZKFHE_PROFILE", "ZKFHE_EARLY_P1", "ZKFHE_WITNESS", "ZKFHE_UPLOAD", "ZKFHE_BI_CHUNK"):
        monkeypatch.delenv(v, raising=False)
    prm = C.BfvParams(N=8)
    inp = synth_input(8, prm.Q, prm.T, prm.B, 1)
    circ = H.BfvCircuit(inp, prm)
    hcfg = H.auto_config(9, 9, circ, transcript=transcript)
    srs_o = H.make_srs(9)
    pk_o, _ = H.keygen_circuit(hcfg, circ, srs_o)
    proof_o, inst_o = H.prove(hcfg, pk_o, srs_o, circ, b"seed-1")
    srs = zk.Srs(ctx, 9)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inp), (8, prm.Q, prm.T, prm.B),
                          zk.BfvConfig(9, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 9, transcript=transcript))
    text = json.dumps(inp)
    launches = {}
    try:
        pk.prove(text, b"warm-up")   # the first proof of a context also creates the auxiliary context's tables
        for name, gate, profile in (("gate 0", 0, None), ("gate 4", 4, None), ("latency under gate 4", 4, "latency"), ("throughput under gate 0", 0, "throughput")):
            zk.prover_gate(gate)
            if profile is None:
                monkeypatch.delenv("ZKFHE_PROFILE", raising=False)
            else:
                monkeypatch.setenv("ZKFHE_PROFILE", profile)
            proof, inst, _ = pk.prove(text, b"seed-1")
            launches[name] = ctx.last_proof_commands()["kernel_launches"]
            assert inst == inst_o, name
            assert first_diff(proof, proof_o) is None, "%s: first differing 32-byte item: %s" % (name, first_diff(proof, proof_o))
    finally:
        zk.prover_gate(0)
        pk.destroy()
        srs.destroy()
    print("transcript %s, kernel launches: %s" % (transcript, launches))
    assert launches["gate 4"] == launches["throughput under gate 0"]
    assert launches["gate 0"] == launches["latency under gate 4"]
    if transcript == "poseidon":
        assert launches["gate 4"] < launches["gate 0"], launches
    else:
        assert launches["gate 4"] == launches["gate 0"], launches   # no early commitment to leave out, and the chunk length is no launch


def test_k13_proof_under_the_gate_matches_oracle_in_59_launches(monkeypatch):
    """One k = 13 proof of the reference's bfv.in under gate 4, on the table budget bench.py's path has (every commitment a sum of
    table points: the suite's 4 GB budget sends the wide ones through the bucket pipeline, whose launches are not this chain's): the
    oracle's bytes, at most 59 kernel launches in steady state -- the chain without the early phase-1 commitment --, no copy, no fill."""
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    for v in ("ZKFHE_PROFILE", "ZKFHE_EARLY_P1", "ZKFHE_WITNESS", "ZKFHE_UPLOAD", "ZKFHE_BI_CHUNK", "ZKFHE_CHAIN"):
        monkeypatch.delenv(v, raising=False)
    saved = {k: os.environ.pop(k, None) for k in ("ZKFHE_TABLE_GB", "ZKFHE_TABLE_BITS")}
    ctx = zk.Context(0)
    try:
        srs = zk.Srs(ctx, 13)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    assert srs.table_bits()[1], "the k = 13 SRS has no table for wide commitments"
    o = oracle_k13()
    pk = zk.BfvProvingKey(ctx, srs, o["text_empty"], (1024, o["prm"].Q, o["prm"].T, o["prm"].B), zk.BfvConfig.from_pinning(o["cfgj"]))
    try:
        zk.prover_gate(4)
        pk.prove(o["text"], b"warm-up")
        proof, inst, _ = pk.prove(o["text"], b"seed-1")
        cmds = ctx.last_proof_commands()
    finally:
        zk.prover_gate(0)
        pk.destroy()
        srs.destroy()
        ctx.close()
    print("k = 13 under gate 4, steady state: %s" % cmds)
    assert inst == o["inst_o"]
    assert first_diff(proof, o["proof_o"]) is None, "first differing 32-byte item: %s" % first_diff(proof, o["proof_o"])
    assert cmds["kernel_launches"] <= 59, cmds
    assert cmds["copy_commands"] == 0 and cmds["fill_commands"] == 0, cmds
