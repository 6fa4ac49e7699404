"""BFV key generation, encryption and decryption on the GPU (bfv_enc.hip) and proofs from machine words
(zkfhe_bfv_prove_words): the ternary negacyclic product against an exact host product, every sample restated from
zk.chacha20_block and the exported error table, ciphertexts against the formula of zk_fhe_amd.inputs, circuit acceptance, and
proofs byte for byte against the JSON path.  Run on the MI355X box: pytest -m gpu."""
import json
import os

import numpy as np
import pytest

from oracle import circuit_ref as C
from oracle import halo2_ref as H

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "bfv")
Q29, Q60, Q63 = 536870909, (1 << 60) - 93, (1 << 63) - 25
SIGMA = 3.2


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


# ---- host restatements -----------------------------------------------------------------------------------------------------

def negacyclic(a, s, q):
    """a * s mod (x^N + 1, q), exact: CircuitInput order in and out; a below 2^64, s in {0, 1, q - 1}.  Each 16-bit limb of a is
    convolved with the centred s in float64 (|terms| < 2^31: exact after rounding), the limbs recombined as Python integers."""
    a = np.asarray(a, dtype=np.uint64)[::-1]
    s = np.asarray(s, dtype=np.uint64)[::-1]
    n = a.size
    sc = np.where(s == 1, 1.0, np.where(s == np.uint64(q - 1), -1.0, 0.0))
    fs = np.fft.rfft(sc, 2 * n)
    total = np.zeros(2 * n, dtype=object)
    for k in range(4):
        limb = ((a >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.float64)
        conv = np.fft.irfft(np.fft.rfft(limb, 2 * n) * fs, 2 * n)
        r = np.rint(conv)
        assert np.abs(conv - r).max() < 0.25
        total += r.astype(np.int64).astype(object) * (1 << (16 * k))
    c = total[:n] - total[n:]
    return np.array([int(x) % q for x in c][::-1], dtype=np.uint64)


def negacyclic_bigint(a, s, q, coeffs):
    """coefficient positions `coeffs` (CircuitInput order) of a * s, by the schoolbook sum in Python integers"""
    n = len(a)
    A = [int(x) for x in a[::-1]]
    S = [1 if int(x) == 1 else (-1 if int(x) == q - 1 else 0) for x in s[::-1]]
    out = []
    for pos in coeffs:
        k = n - 1 - pos
        v = sum(A[i] * S[k - i] for i in range(k + 1)) - sum(A[i] * S[n + k - i] for i in range(k + 1, n))
        out.append(v % q)
    return out


def words(seed, domain, index, n_words):
    import zk_fhe_amd as zk
    out = []
    for blk in range((n_words + 7) // 8):
        b = zk.chacha20_block(seed, [blk, domain, index & 0xFFFFFFFF, index >> 32])
        out += [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(8)]
    return out[:n_words]


def ternary(seed, domain, index, n, q):
    return np.array([((w * 3 >> 64) - 1) % q for w in words(seed, domain, index, n)], dtype=np.uint64)


def uniform(seed, domain, index, n, q):
    w = words(seed, domain, index, 2 * n)
    return np.array([((w[2 * p] | w[2 * p + 1] << 64) * q) >> 128 for p in range(n)], dtype=np.uint64)


def error(seed, domain, index, n, q, b):
    import zk_fhe_amd as zk
    cdt = zk.bfv_error_cdt((8, q, 2, b))
    w = np.array(words(seed, domain, index, n), dtype=np.uint64)
    x = np.searchsorted(cdt, w, side="right").astype(np.int64) - b   # #{i : T_i <= w} - B
    return np.array([int(v) % q for v in x], dtype=np.uint64)


def centred(v, q):
    v = np.asarray(v, dtype=np.uint64).astype(object)
    return np.array([int(x) - q if int(x) > q // 2 else int(x) for x in v], dtype=object)


def random_m(rng, shape, q, t):
    """messages centred in (-T/2, T/2] (for even T, -T/2 and T/2 are one residue mod T)"""
    m = rng.integers(-((t - 1) // 2), t // 2 + 1, size=shape, dtype=np.int64)
    return np.array([int(x) % q for x in m.reshape(-1)], dtype=np.uint64).reshape(shape)


def to_json(pk0, pk1, m, ct, j=0):
    n = len(pk0)
    st = lambda v: [str(int(x)) for x in v]  # noqa: E731
    cyclo = [1] + [0] * (n - 1) + [1]
    return json.dumps(dict(pk0=st(pk0), pk1=st(pk1), m=st(m), u=st(ct["u"][j]), e0=st(ct["e0"][j]), e1=st(ct["e1"][j]),
                           c0=st(ct["c0"][j]), c1=st(ct["c1"][j]), cyclo=st(cyclo)))


# ---- 1. product parity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 1024, 4096, 16384, 32768])
@pytest.mark.parametrize("q", [Q29, Q60, Q63])
def test_product_parity(ctx, n, q):
    rng = np.random.default_rng(n ^ q)
    a = rng.integers(0, q, size=(2, n), dtype=np.uint64)
    s = rng.choice(np.array([0, 1, q - 1], dtype=np.uint64), size=(2, n))
    shared = ctx.poly_mul_ternary_negacyclic(a[0], s, q)
    per = ctx.poly_mul_ternary_negacyclic(a, s, q)
    for j in range(2):
        assert np.array_equal(shared[j], negacyclic(a[0], s[j], q)), j
        assert np.array_equal(per[j], negacyclic(a[j], s[j], q)), j
    pos = [0, 1, n // 2, n - 1] if n > 8 else list(range(8))
    assert [int(per[1][p]) for p in pos] == negacyclic_bigint(a[1], s[1], q, pos)


@pytest.mark.parametrize("n", [8, 32768])
def test_product_crt_range_extremes(ctx, n):
    for q in (Q29, Q63):
        a = np.full(n, q - 1, dtype=np.uint64)
        for sv in (1, q - 1):
            s = np.full((1, n), sv, dtype=np.uint64)
            got = ctx.poly_mul_ternary_negacyclic(a, s, q)[0]
            assert np.array_equal(got, negacyclic(a, s[0], q))
            pos = [0, n - 1]
            assert [int(got[p]) for p in pos] == negacyclic_bigint(a, s[0], q, pos)


def test_product_refuses_non_ternary(ctx):
    import zk_fhe_amd as zk
    n, q = 1024, Q60
    a = np.ones(n, dtype=np.uint64)
    s = np.zeros((2, n), dtype=np.uint64)
    s[1, 17] = 2
    with pytest.raises(zk.ZkfheError, match="not in"):
        ctx.poly_mul_ternary_negacyclic(a, s, q)
    s[1, 17] = q - 2
    with pytest.raises(zk.ZkfheError):
        ctx.poly_mul_ternary_negacyclic(a, s, q)
    s[1, 17] = q - 1   # valid again: the context still works
    assert np.array_equal(ctx.poly_mul_ternary_negacyclic(a, s, q)[1], negacyclic(a, s[1], q))


# ---- 2. samplers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,t,b,first", [(1024, Q29, 7, 19, 0), (16384, Q60, 65537, 19, (1 << 32) + 5)])
def test_samples_restate_from_chacha(ctx, n, q, t, b, first):
    prm = (n, q, t, b)
    kseed, eseed = bytes(range(32)), bytes(range(100, 132))
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, kseed)
    assert np.array_equal(sk, ternary(kseed, 4, 0, n, q))
    assert np.array_equal(pk1, uniform(kseed, 5, 0, n, q))
    e = error(kseed, 6, 0, n, q, b)
    assert np.array_equal(pk0, (q - (negacyclic(pk1, sk, q).astype(object) + e.astype(object)) % q) % q)
    m = random_m(np.random.default_rng(1), (2, n), q, t)
    ct = ctx.bfv_encrypt(prm, pk0, pk1, m, eseed, first_index=first)
    for j in range(2):
        assert np.array_equal(ct["u"][j], ternary(eseed, 1, first + j, n, q)), j
        assert np.array_equal(ct["e0"][j], error(eseed, 2, first + j, n, q, b)), j
        assert np.array_equal(ct["e1"][j], error(eseed, 3, first + j, n, q, b)), j
    for k in ("e0", "e1"):
        assert np.abs(centred(ct[k].reshape(-1), q).astype(np.int64)).max() <= b
    assert not np.array_equal(ct["u"][0], ct["u"][1])   # index changes the stream
    other = ctx.bfv_encrypt(prm, pk0, pk1, m[:1], bytes(range(1, 33)), first_index=first)
    assert not np.array_equal(other["u"][0], ct["u"][0]) and not np.array_equal(other["e0"][0], ct["e0"][0])
    again = ctx.bfv_encrypt(prm, pk0, pk1, m[1:], eseed, first_index=first + 1)   # (seed, index) fixes the draw
    assert np.array_equal(again["u"][0], ct["u"][1]) and np.array_equal(again["c0"][0], ct["c0"][1])


def test_error_distribution_chi_square(ctx):
    import zk_fhe_amd as zk
    n, q, t, b = 16384, Q60, 65537, 19
    prm = (n, q, t, b)
    _, pk0, pk1 = ctx.bfv_fhe_keypair(prm, b"\x07" * 32)
    ct = ctx.bfv_encrypt(prm, pk0, pk1, np.zeros((31, n), dtype=np.uint64), b"\x09" * 32)
    x = np.concatenate([centred(ct["e0"].reshape(-1), q), centred(ct["e1"].reshape(-1), q)]).astype(np.int64)
    assert x.size >= 10 ** 6
    support = np.arange(-b, b + 1)
    p = np.exp(-support.astype(np.float64) ** 2 / (2 * SIGMA ** 2))
    p /= p.sum()
    counts = np.array([(x == v).sum() for v in support], dtype=np.float64)
    exp = p * x.size
    keep = exp >= 5
    chi2 = (((counts - exp) ** 2 / exp)[keep]).sum() + ((counts[~keep].sum() - exp[~keep].sum()) ** 2 / max(exp[~keep].sum(), 1e-9) if (~keep).any() else 0)
    dof = int(keep.sum())
    assert chi2 < dof + 8 * np.sqrt(2 * dof), (chi2, dof)
    cdt = zk.bfv_error_cdt(prm)
    assert cdt.size == 2 * b


# ---- 3. ciphertexts --------------------------------------------------------------------------------------------------------

def test_ciphertext_formula(ctx):
    n, q, t, b = 1024, Q29, 7, 19
    prm = (n, q, t, b)
    _, pk0, pk1 = ctx.bfv_fhe_keypair(prm, b"\x01" * 32)
    m = random_m(np.random.default_rng(3), (4, n), q, t)
    ct = ctx.bfv_encrypt(prm, pk0, pk1, m, b"\x02" * 32, first_index=9)
    delta = q // t
    for j in range(4):
        u = ct["u"][j]
        md = np.array([int(x) * delta % q for x in m[j]], dtype=object)
        c0 = (negacyclic(pk0, u, q).astype(object) + md + ct["e0"][j].astype(object)) % q
        c1 = (negacyclic(pk1, u, q).astype(object) + ct["e1"][j].astype(object)) % q
        assert np.array_equal(ct["c0"][j].astype(object), c0), j
        assert np.array_equal(ct["c1"][j].astype(object), c1), j


@pytest.mark.parametrize("n,q,t", [(1024, Q29, 7), (4096, Q60, 65537), (16384, Q60, 65537), (32768, Q63, 1 << 20)])
def test_decrypt_batch_of_64(ctx, n, q, t):
    prm = (n, q, t, 19)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
    m = random_m(np.random.default_rng(n), (64, n), q, t)
    ct = ctx.bfv_encrypt(prm, pk0, pk1, m)
    assert np.array_equal(ctx.bfv_decrypt(prm, sk, ct["c0"], ct["c1"]), m)


def test_out_of_range_inputs_refused(ctx):
    import zk_fhe_amd as zk
    n, q, t, b = 1024, Q29, 7, 19
    prm = (n, q, t, b)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, b"\x03" * 32)
    m = np.zeros((1, n), dtype=np.uint64)
    for v in (t // 2 + 1, q - t // 2 - 1, q, 1 << 62):
        bad = m.copy()
        bad[0, 5] = v
        with pytest.raises(zk.ZkfheError, match="message"):
            ctx.bfv_encrypt(prm, pk0, pk1, bad, b"\x04" * 32)
    for v in (t // 2, q - t // 2, q - 1):   # the range's own ends
        ok = m.copy()
        ok[0, 5] = v
        ct = ctx.bfv_encrypt(prm, pk0, pk1, ok, b"\x04" * 32)
        assert np.array_equal(ctx.bfv_decrypt(prm, sk, ct["c0"], ct["c1"]), ok)
    for which in (0, 1):
        pk = [pk0.copy(), pk1.copy()]
        pk[which][7] = q
        with pytest.raises(zk.ZkfheError, match="public-key"):
            ctx.bfv_encrypt(prm, pk[0], pk[1], m, b"\x04" * 32)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        ctx.bfv_encrypt((n, q, q, b), pk0, pk1, m, b"\x04" * 32)   # T >= Q
    bad_sk = sk.copy()
    bad_sk[3] = 5
    with pytest.raises(zk.ZkfheError, match="secret-key"):
        ctx.bfv_decrypt(prm, bad_sk, np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64))


# ---- 4. circuit acceptance -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 1024])
def test_gpu_encryption_satisfies_the_circuit(ctx, n):
    import zk_fhe_amd as zk
    prm = C.BfvParams(N=n)
    params = (n, prm.Q, prm.T, prm.B)
    _, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x05" * 32)
    m = random_m(np.random.default_rng(5), (1, n), prm.Q, prm.T)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x06" * 32)
    text = to_json(pk0, pk1, m[0], ct)
    if n == 8:
        hcfg = H.auto_config(9, 9, H.BfvCircuit(json.loads(text), prm))
        cfg = zk.BfvConfig(9, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 9)
    else:
        cfg = zk.bfv_auto_config(text, params, 13)
    fails, first = zk.bfv_mock(text, params, cfg)
    assert fails == 0, first


# ---- 5. same bytes ---------------------------------------------------------------------------------------------------------

def split_json(text):
    d = json.loads(text)
    return {k: np.array([int(x) for x in d[k]], dtype=np.uint64) for k in ("pk0", "pk1", "m", "u", "e0", "e1", "c0", "c1")}


@pytest.mark.parametrize("transcript", ["poseidon", "blake2b"])
def test_prove_words_toy_same_bytes(ctx, transcript):
    import zk_fhe_amd as zk
    from tests.test_proof_oracle import synth_input
    prm = C.BfvParams(N=8)
    inp = synth_input(8, prm.Q, prm.T, prm.B, 1)
    circ = H.BfvCircuit(inp, prm)
    hcfg = H.auto_config(9, 9, circ, transcript=transcript)
    srs_o = H.make_srs(9)
    pk_o, _ = H.keygen_circuit(hcfg, circ, srs_o)
    srs = zk.Srs(ctx, 9)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inp), (8, prm.Q, prm.T, prm.B),
                          zk.BfvConfig(9, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 9, transcript=transcript))
    try:
        text = json.dumps(inp)
        proof, inst, _ = pk.prove(text, b"seed-w")
        proof_w, inst_w, _ = pk.prove_words(split_json(text), b"seed-w")
        assert proof_w == proof and list(inst_w) == list(inst)
        assert H.verify(H.VerifyingKey(pk_o), srs_o, inst_w, proof_w)
        ok, why = zk.bfv_verify(pk.export_vk(), inst_w, proof_w)
        assert ok, why
    finally:
        pk.destroy()
        srs.destroy()


@pytest.fixture(scope="module")
def key13(ctx):
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    cfgj = json.load(open(os.path.join(G, "bfv_config.json")))
    prm = C.BfvParams()
    params = (1024, prm.Q, prm.T, prm.B)
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), params, zk.BfvConfig.from_pinning(cfgj), replay=True)
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(params, b"\x0b" * 32)
    yield dict(pk=pk, params=params, sk=sk, pk0=pk0, pk1=pk1)
    pk.destroy()
    srs.destroy()


def test_prove_words_k13_same_bytes_and_refusals(ctx, key13):
    import zk_fhe_amd as zk
    pk, params, pk0, pk1 = key13["pk"], key13["params"], key13["pk0"], key13["pk1"]
    q, t = params[1], params[2]
    m = random_m(np.random.default_rng(13), (2, 1024), q, t)
    ct = ctx.bfv_encrypt(params, pk0, pk1, m, b"\x0c" * 32)
    before = pk.prefix_cache()
    for j in range(2):
        text = to_json(pk0, pk1, m[j], ct, j)
        proof, inst, _ = pk.prove(text, b"k13-%d" % j)
        proof_w, inst_w, tm = pk.prove_words(split_json(text), b"k13-%d" % j)
        assert proof_w == proof and list(inst_w) == list(inst), j
        assert len(tm) == 5 and tm[4] > 0
        ok, why = zk.bfv_verify(pk.export_vk(), inst_w, proof_w)
        assert ok, why
    after = pk.prefix_cache()
    assert after["hits"] >= before["hits"] + 3   # every proof after the first under this public key starts from the cached state
    # a tampered c0 word: the same refusal as the text path
    text = to_json(pk0, pk1, m[0], ct)
    w = split_json(text)
    w["c0"][1] = (int(w["c0"][1]) + 1) % q
    bad_text = json.loads(text)
    bad_text["c0"][1] = str(int(w["c0"][1]))
    with pytest.raises(zk.ZkfheError) as e_text:
        pk.prove(json.dumps(bad_text), b"bad")
    with pytest.raises(zk.ZkfheError) as e_words:
        pk.prove_words(w, b"bad")
    assert str(e_words.value) == str(e_text.value)
    # a word above Q leaves the machine-word path: rendered as JSON, refused the text path's way
    w = split_json(text)
    w["m"][0] = q + 5
    bad_text = json.loads(text)
    bad_text["m"][0] = str(q + 5)
    with pytest.raises(zk.ZkfheError) as e_text:
        pk.prove(json.dumps(bad_text), b"bad")
    with pytest.raises(zk.ZkfheError) as e_words:
        pk.prove_words(w, b"bad")
    assert str(e_words.value) == str(e_text.value)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------

def test_encrypt_and_prove_sixteen(ctx, key13):
    import zk_fhe_amd as zk
    pk, params, sk, pk0, pk1 = key13["pk"], key13["params"], key13["sk"], key13["pk0"], key13["pk1"]
    m = random_m(np.random.default_rng(16), (16, 1024), params[1], params[2])
    c0, c1, proofs, insts = pk.encrypt_and_prove(pk0, pk1, m)
    assert len(proofs) == 16
    res = zk.bfv_verify_batch(ctx, pk.export_vk(), list(zip(insts, proofs)))
    assert all(ok for ok, _ in res), [why for ok, why in res if not ok]
    assert np.array_equal(ctx.bfv_decrypt(params, sk, c0, c1), m)
    n = params[0]
    for j in (0, 15):   # the public inputs carry this ciphertext: pk0 | pk1 | c0 | c1 | cyclo
        inst = list(insts[j])
        assert inst[2 * n:3 * n] == [int(x) for x in c0[j]] and inst[3 * n:4 * n] == [int(x) for x in c1[j]]
    c0s, c1s, proof1, inst1 = pk.encrypt_and_prove(pk0, pk1, m[0], enc_seed=b"\x0d" * 32, seed=b"one")
    assert c0s.shape == (n,) and zk.bfv_verify(pk.export_vk(), inst1, proof1)[0]
