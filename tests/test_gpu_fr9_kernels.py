"""The kernels that moved to the nine-limb Fr value (zk-fhe_amd/csrc/fr9.hip.hpp) on the device: its operations as the kernels compose
them, element by element over an operand grid (zkfhe_fr9_op) against Python integers; the batch inversion at the sizes where its
chains begin, end and change length; and proofs of the smallest circuits the prover accepts, byte for byte against the oracle prover
-- they run every group type of k_quotient_partials, and k_lookup_num_den and k_prefix_product.
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import json
import os

import numpy as np
import pytest

from oracle import binding as orc
from oracle import circuit_ref as C
from oracle import halo2_ref as H
from oracle import pyref
from tests.test_gpu_fr_edges import WORDS, plant_zeros
from tests.test_proof_oracle import synth_input

pytestmark = pytest.mark.gpu
R = pyref.R
RINV = pow(1 << 256, -1, R)   # the words in memory are x 2^256: the product of two words is a b / 2^256
# the operand words of tests/test_gpu_fr_edges.py, and 2^k - 1 at the limb boundaries of both radices
GRID = sorted(set(WORDS) | {0, 1, R - 1, R - 2} | {(1 << k) - 1 for k in (5, 24, 29, 58, 227, 232, 253)})
M = len(GRID)
# every ordered pair (a, b); c, d, e walk the words at other strides, so every word meets every position
TUPLES = [(GRID[i], GRID[j], GRID[(i + j) % M], GRID[(i + 2 * j + 1) % M], GRID[(2 * i + j + 3) % M]) for i in range(M) for j in range(M)]
OPS = {
    "mul": lambda a, b, c, d, e: a * b * RINV % R,
    "sqr": lambda a, b, c, d, e: a * a * RINV % R,
    "mul2": lambda a, b, c, d, e: (a * b + c * d) * RINV % R,
    "perm": lambda a, b, c, d, e: a * (b + c * d * RINV + e) * RINV % R,      # a step of a permutation product
    "lookup": lambda a, b, c, d, e: (a + b) * (c + d) * RINV % R,            # a term of the lookup argument
    "chain": lambda a, b, c, d, e: a * b * c * RINV * RINV % R,              # a product regrouped in registers as the next one's constant
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
def operands():
    return [orc.ints_to_arr([t[k] for t in TUPLES]) for k in range(5)]


@pytest.fixture(scope="module")
def expected():
    return {op: orc.ints_to_arr([f(*t) for t in TUPLES]) for op, f in OPS.items()}


def test_the_grid_is_canonical_and_every_word_meets_every_position():
    assert all(0 <= w < R for w in GRID) and M >= 18
    for k in range(5):
        assert {t[k] for t in TUPLES} == set(GRID)


@pytest.mark.parametrize("op", sorted(OPS))
def test_fr9_operations_on_the_operand_grid(ctx, operands, expected, op):
    """n = 1, 63, 64, 65 (a wave and its neighbours), the whole grid of tuples, and two full launches of the element-wise kernels and three
    elements more, so that every thread takes its grid stride"""
    L = len(TUPLES)
    two_grids = 2 * (ctx.device_info()["num_cu"] * 8 * 256) + 3
    assert two_grids >= 2 * 256 * 8 + 3
    for n in (1, 63, 64, 65, L, two_grids):
        reps = -(-n // L)
        ins = [np.tile(o, (reps, 1))[:n] for o in operands]
        got = ctx.fr9_op(op, ins)
        assert np.array_equal(got, np.tile(expected[op], (reps, 1))[:n]), (op, n)


def inverse_words(words):
    """x^-1 as a word: (w / 2^256)^(r - 2) 2^256, zero staying zero"""
    return [pow(w * RINV % R, R - 2, R) * (1 << 256) % R for w in words]


@pytest.fixture(scope="module")
def long_words():
    """2^20 + 5 canonical words and as many numerators; r - 1 and 1 among the denominators"""
    rng = np.random.default_rng(99)
    w = rng.integers(0, 1 << 63, size=(2, (1 << 20) + 5, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(2, (1 << 20) + 5, 4), dtype=np.uint64)
    w[:, :, 3] &= np.uint64((1 << 60) - 1)
    w[0, :, 0] |= np.uint64(1)   # no accidental zero among the denominators
    w[0, 5::1000] = orc.ints_to_arr([(R - 1) * (1 << 256) % R])[0]
    w[0, 6::1000] = orc.ints_to_arr([(1 << 256) % R])[0]
    return w[0], w[1]


@pytest.mark.parametrize("n", [1, 7, 8, 9, (1 << 11) + 1])
def test_batch_invert_at_the_ends_of_a_chain(ctx, n):
    """one element, one thread's chain of eight less one, exactly, plus one, and 2^11 + 1; zeros first, last and through a whole thread's
    stride; the values r - 1 and 1; against pow(x, r - 2, r)"""
    rng = np.random.default_rng(n)
    one = (1 << 256) % R
    words = [int.from_bytes(rng.bytes(32), "little") % R or 1 for _ in range(n)]
    words[n // 2] = (R - 1) * one % R
    if n > 2:
        words[1] = one
    T = -(-n // 8)   # threads of the launch: thread t owns t, t + T, t + 2 T, ...
    for zeros in ((), (0,), (n - 1,), (0, n - 1), tuple(range(min(3, T - 1), n, T))):   # the last: one thread's whole chain
        w = list(words)
        for z in zeros:
            w[z] = 0
        den = orc.ints_to_arr(w)
        want = inverse_words(w)
        assert all(0 <= x < R for x in want) and [x == 0 for x in want] == [x == 0 for x in w]
        assert orc.arr_to_ints(ctx.fr_unop("batch_invert", den)) == want, (n, zeros)
        num = orc.ints_to_arr(words[::-1])
        assert orc.arr_to_ints(ctx.fr_batch_invert_mul(num, den)) == [a * b * RINV % R for a, b in zip(words[::-1], want)], (n, zeros)


@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20])
def test_batch_invert_on_both_sides_of_the_long_array_threshold(ctx, long_words, n):
    """eight elements per inversion below 2^20, at least sixteen from there on: the oracle on every element, pow(x, r - 2, r) on the first
    and last 48 and on the planted words"""
    den, zero = plant_zeros(long_words[0][:n])
    num = long_words[1][:n]
    inv = ctx.fr_unop("batch_invert", den)
    assert np.array_equal(inv, orc.fr_batch_inv(den))
    assert not inv[zero].any() and inv[~zero].any(axis=1).all()
    sample = list(range(48)) + list(range(n - 48, n)) + [1005, 2005, 2006]
    assert orc.arr_to_ints(inv[sample]) == inverse_words(orc.arr_to_ints(den[sample]))
    quot = ctx.fr_batch_invert_mul(num, den)
    assert np.array_equal(quot, orc.fe_binop("mul", num, inv))
    assert not quot[zero].any()


def prove_and_compare(ctx, N, k, unusable, inp, seed, transcript="poseidon"):
    import zk_fhe_amd as zk
    prm = C.BfvParams(N=N)
    circ = H.BfvCircuit(inp, prm)
    hcfg = H.auto_config(k, unusable, circ, transcript=transcript)
    srs_o = H.make_srs(k)
    pk_o, _ = H.keygen_circuit(hcfg, circ, srs_o)
    proof_o, inst_o = H.prove(hcfg, pk_o, srs_o, circ, seed)
    srs = zk.Srs(ctx, k)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inp), (N, prm.Q, prm.T, prm.B),
                          zk.BfvConfig(k, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, unusable, transcript=transcript))
    try:
        assert pk.info()["vk_digest"] == pk_o.vk_digest
        proof, inst, _ = pk.prove(json.dumps(inp), seed)
        assert inst == inst_o
        assert proof == proof_o, "the proof bytes differ from the oracle prover's"
        ok, why = zk.bfv_verify(pk.export_vk(), inst, proof)
        assert ok, why
    finally:
        pk.destroy()
        srs.destroy()


@pytest.mark.parametrize("transcript", ["poseidon", "blake2b"])
def test_toy_proof_bytes(ctx, transcript):
    """N = 8 in 2^9 rows: every quotient group type and the grand-product kernels at the smallest size the prover accepts"""
    prm = C.BfvParams(N=8)
    prove_and_compare(ctx, 8, 9, 9, synth_input(8, prm.Q, prm.T, prm.B, 1), b"fr9", transcript)


def test_k14_proof_bytes(ctx):
    """N = 16 in 2^14 rows, an encryption drawn by zk_fhe_amd.inputs under the plaintext modulus and error bound of tests/golden/bfv"""
    from zk_fhe_amd import inputs
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfv", "bfv.in")))
    prm = C.BfvParams(N=16)
    assert len(ref["pk0"]) == 1024 and max(int(x) for x in ref["pk0"]) < prm.Q
    prove_and_compare(ctx, 16, 14, 109, inputs.generate(n=16, q=prm.Q, t=prm.T, b=prm.B, seed=14), b"fr9-k14")
