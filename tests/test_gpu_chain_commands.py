"""The command chain of a proof (zkfhe_ctx_last_proof_commands) and what was fused to shorten it: a k = 13 proof in steady state
puts kernels on its streams and nothing else -- no copy and no fill command --, its bytes are still the oracle's, a context that is
reused or that saw a rejected witness carries no state over, the inversion with a numerator equals invert-then-multiply, and two
streams proving at once give the sequential bytes.  Run on the MI355X box: pytest -m gpu."""
import copy
import hashlib
import json
import os
import threading

import numpy as np
import pytest

from oracle import circuit_ref as C
from oracle import halo2_ref as H
from tests.test_gpu_prover import first_diff, oracle_k13
from tests.test_proof_oracle import synth_input

pytestmark = pytest.mark.gpu
SEED = b"seed-1"   # the seed of oracle_k13's proof


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


_ORACLE_BLAKE2B = {}


def oracle_k13_proof(transcript):
    """(proof, instances) of the reference's bfv.in by the CPU oracle at the pinned k = 13 layout.  Poseidon: the session's shared
    oracle_k13().  Blake2b: the same key -- fixed and permutation commitments do not depend on the transcript, the vk digest does
    and is recomputed by keygen_circuit's rule -- and one more oracle proof, made once."""
    o = oracle_k13()
    if transcript == "poseidon":
        return o["proof_o"], o["inst_o"]
    if not _ORACLE_BLAKE2B:
        hcfg = H.Config.from_pinning(o["cfgj"], transcript="blake2b")
        pk_b = copy.copy(o["pk_o"])
        pk_b.cfg = hcfg
        h =hashlib.blake2b(digest_size=64, person=b"zkfhe-vk")
        for v in (hcfg.k, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, hcfg.unusable_rows, hcfg.lookup_bits, H.TRANSCRIPT_ID["blake2b"]):
            h.update(int(v).to_bytes(4, "little"))
        for P in pk_b.fixed_commit + pk_b.sigma_commit:
            x, y = (0, 0) if P is None else P
            h.update(x.to_bytes(32, "little") + y.to_bytes(32, "little"))
        pk_b.vk_digest = H.from_bytes_wide(h.digest())
        proof, inst = H.prove(hcfg, pk_b, o["srs_o"], H.BfvCircuit(json.loads(o["text"]), o["prm"]), SEED)
        assert H.verify(H.VerifyingKey(pk_b), o["srs_o"], inst, proof)
        _ORACLE_BLAKE2B.update(proof=proof, inst=inst, vk_digest=pk_b.vk_digest)
    return _ORACLE_BLAKE2B["proof"], _ORACLE_BLAKE2B["inst"]


@pytest.fixture(scope="module")
def k13(ctx):
    """One k = 13 SRS with the library's default table budget -- digit-multiple tables wide enough for every commitment, the path
    bench.py measures (the suite's 4 GB budget sends the wide commitments through the bucket pipeline) -- and one key per transcript."""
    import zk_fhe_amd as zk
    saved = {k: os.environ.pop(k, None) for k in ("ZKFHE_TABLE_GB", "ZKFHE_TABLE_BITS")}
    try:
        srs = zk.Srs(ctx, 13)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    assert srs.table_bits()[1], "the k = 13 SRS has no table for wide commitments"
    o = oracle_k13()
    keys = {}

    def key(transcript):
        if transcript not in keys:
            zcfg = zk.BfvConfig.from_pinning(o["cfgj"], transcript=transcript)
            keys[transcript] = zk.BfvProvingKey(ctx, srs, o["text_empty"], (1024, o["prm"].Q, o["prm"].T, o["prm"].B), zcfg)
        return keys[transcript]
    yield key
    for pk in keys.values():
        pk.destroy()
    srs.destroy()


@pytest.mark.parametrize("early", ["0", "1"])
@pytest.mark.parametrize("transcript", ["poseidon", "blake2b"])
def test_k13_proof_is_kernels_only_and_matches_oracle(ctx, k13, monkeypatch, transcript, early):
    """A k = 13 proof of the default path, both transcripts, early phase-1 commitment off and on: 0 copy commands, 0 fill commands,
    the oracle's bytes.  Counted on the second proof of the context: the first one also creates the auxiliary context's tables."""
    monkeypatch.setenv("ZKFHE_EARLY_P1", early)
    monkeypatch.delenv("ZKFHE_WITNESS", raising=False)
    monkeypatch.delenv("ZKFHE_UPLOAD", raising=False)
    o = oracle_k13()
    proof_o, inst_o = oracle_k13_proof(transcript)
    pk = k13(transcript)
    pk.prove(o["text"], b"warm-up")
    first = ctx.last_proof_commands()
    proof, inst, _ = pk.prove(o["text"], SEED)
    cmds = ctx.last_proof_commands()
    print("transcript %s, ZKFHE_EARLY_P1=%s: first proof on the context %s, steady state %s" % (transcript, early, first, cmds))
    assert cmds["kernel_launches"] > 20
    assert cmds["copy_commands"] == 0, cmds
    assert cmds["fill_commands"] == 0, cmds
    assert inst == inst_o
    assert first_diff(proof, proof_o) is None, "first differing 32-byte item: %s" % first_diff(proof, proof_o)


def toy(transcript="poseidon"):
    """the toy configuration of test_toy_proof_bytes_match_oracle: N = 8 ring, k = 9 circuit"""
    prm = C.BfvParams(N=8)
    inputs = [synth_input(8, prm.Q, prm.T, prm.B, s) for s in (1, 2, 3, 4)]
    hcfg = H.auto_config(9, 9, H.BfvCircuit(inputs[0], prm), transcript=transcript)
    return prm, inputs, hcfg


@pytest.mark.parametrize("transcript", ["poseidon", "blake2b"])
def test_reused_context_gives_the_same_bytes(ctx, transcript):
    """Input A, input B, input A again on one context: the third proof is the first one, byte for byte -- nothing a proof leaves
    behind in the workspace (instance column, staging ring, columns cleared or blinded by a neighbouring kernel) reaches the next."""
    import zk_fhe_amd as zk
    prm, inputs, hcfg = toy(transcript)
    srs = zk.Srs(ctx, 9)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs[0]), (8, prm.Q, prm.T, prm.B),
                          zk.BfvConfig(9, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 9, transcript=transcript))
    a1, inst_a1, _ = pk.prove(json.dumps(inputs[0]), b"reuse-a")
    b, inst_b, _ = pk.prove(json.dumps(inputs[1]), b"reuse-b")
    a2, inst_a2, _ = pk.prove(json.dumps(inputs[0]), b"reuse-a")
    assert b != a1 and inst_b != inst_a1
    assert inst_a2 == inst_a1
    assert first_diff(a2, a1) is None, "first differing 32-byte item: %s" % first_diff(a2, a1)
    ok, why = zk.bfv_verify(pk.export_vk(), inst_a2, a2)
    assert ok, why
    pk.destroy()
    srs.destroy()


def test_valid_proof_after_a_rejected_witness_matches_oracle(ctx, k13):
    """The first rejected input of test_generated_inputs_and_rejected_witnesses (e0 outside [-B, B]) ends its proof early, at the
    permutation argument; the valid proof on the same context right after has the oracle's bytes."""
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    o = oracle_k13()
    prm = o["prm"]
    pk = k13("poseidon")
    bad = inputs.generate(1024, prm.Q, prm.T, prm.B, seed=5)
    e0 = list(bad["e0"])
    e0[7] = str(prm.B + 1)
    bad["e0"] = e0
    with pytest.raises(zk.ZkfheError):
        pk.prove(json.dumps(bad), b"gen-5")
    proof, inst, _ = pk.prove(o["text"], SEED)
    assert inst == o["inst_o"]
    assert first_diff(proof, o["proof_o"]) is None, "first differing 32-byte item: %s" % first_diff(proof, o["proof_o"])


@pytest.mark.parametrize("n", [1, 7, 8, 9, (1 << 11) + 3])
def test_batch_invert_with_numerator(ctx, n):
    """zkfhe_fr_batch_invert_mul against zkfhe_fr_batch_invert followed by zkfhe_fr_mul, and against num * den^-1 on integers.
    A thread inverts a group of 8 elements: the lengths fall short of one group, fill it, exceed it, and leave a ragged last
    group.  One denominator is zero: the plain call leaves it zero, so the quotient there is zero."""
    from oracle import binding as orc
    from oracle import pyref
    rng = np.random.default_rng(n)
    num = [int.from_bytes(rng.bytes(32), "little") % pyref.R for _ in range(n)]
    den = [int.from_bytes(rng.bytes(32), "little") % pyref.R or 1 for _ in range(n)]
    den[n // 2] = 0
    num_m, den_m = orc.ints_to_mont(num), orc.ints_to_mont(den)
    got = ctx.fr_batch_invert_mul(num_m, den_m)
    two_calls = ctx.fr_binop("mul", num_m, ctx.fr_unop("batch_invert", den_m))
    want = orc.ints_to_mont([a * pow(b, -1, pyref.R) % pyref.R if b else 0 for a, b in zip(num, den)])
    assert np.array_equal(got, two_calls)
    assert np.array_equal(got, np.asarray(want).reshape(got.shape))


def test_two_streams_at_once_match_sequential(ctx):
    """Two contexts prove different inputs against one key at the same time: the bytes each input gives alone."""
    import zk_fhe_amd as zk
    prm, inputs, hcfg = toy()
    srs = zk.Srs(ctx, 9)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs[0]), (8, prm.Q, prm.T, prm.B), zk.BfvConfig(9, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 9))
    alone = [pk.prove(json.dumps(i), b"s%d" % k)[0] for k, i in enumerate(inputs)]
    ctx2 = zk.Context(0)
    got = [None] * 4
    errors = []

    def work(c, ks):
        try:
            for _ in range(2):
                for k in ks:
                    got[k] = pk.prove(json.dumps(inputs[k]), b"s%d" % k, ctx=c)[0]
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(ctx, (0, 1))), threading.Thread(target=work, args=(ctx2, (2, 3)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == alone
    pk.destroy()
    srs.destroy()
    ctx2.close()
