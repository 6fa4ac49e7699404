"""Host side of the baby-step/giant-step linear transform (no GPU): a pure-Python restatement of zkfhe_bfv_linear_transform_bsgs from
zkfhe.h on the restatements of tests/test_bfv_linear_host.py, bit-equal to their composition; a dense 16 x 16 (and one 64 x 64) matrix
through zk.bfv_matrix_bsgs and the restated call decrypts to M v; the helper alone on slot values against matrix @ v, its dropped
rows and columns and its element lists; the declaration, export and mirror.  tests/test_gpu_bfv_bsgs.py imports the restatement."""
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, deg, circ, kron_negacyclic, relin_digits
from tests.test_bfv_galois_host import encode, eval_slots, galois_element, ref_galois_key, rotate, sigma
from tests.test_bfv_linear_host import ref_hoisted_rotation, ref_linear_transform, sigma_z
from tests.test_bfv_threshold_host import ref_decrypt, ref_encrypt, ref_keygen_share, ref_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition, restated from zkfhe.h ---------------------------------------------------------------------------------

def ref_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag):
    """zkfhe_bfv_linear_transform_bsgs of one ciphertext: inner_i = the linear transform over the baby elements with diag[i], mod Q
    into [0, Q); out = sum_i (hoisted rotation of inner_i by g_giant[i]) exactly over Z, then mod Q.  The integer sum is written out
    here: sigma_g(inner0) plus the digit products with the key rows for g != 1, (inner0, inner1) itself for g = 1."""
    n, q = params[0], params[1]
    l = relin_digits(q, w)
    acc0, acc1 = [0] * n, [0] * n
    for i, g in enumerate(g_giant):
        in0, in1 = ref_linear_transform(params, c0, c1, g_baby, bk0, bk1, w, diag[i])
        if g == 1:
            r0, r1 = deg(in0), deg(in1)
        else:
            d1 = deg(in1)
            digits = [sigma_z([(c >> (k * w)) & ((1 << w) - 1) for c in d1], g) for k in range(l)]
            r0 = [x + y for x, y in zip(deg(sigma(in0, g, q)), kron_negacyclic([(digits[k], deg(hk0[i][k])) for k in range(l)], n))]
            r1 = kron_negacyclic([(digits[k], deg(hk1[i][k])) for k in range(l)], n)
        acc0 = [x + y for x, y in zip(acc0, r0)]
        acc1 = [x + y for x, y in zip(acc1, r1)]
    return circ(acc0, q), circ(acc1, q)


def composed(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag):
    """the same through the two sibling restatements and a sum mod Q"""
    n, q = params[0], params[1]
    acc = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]
    for i, g in enumerate(g_giant):
        inner = ref_linear_transform(params, c0, c1, g_baby, bk0, bk1, w, diag[i])
        r = ref_hoisted_rotation(params, inner[0], inner[1], g, hk0[i], hk1[i], w)
        acc = [np.array([(int(a) + int(b)) % q for a, b in zip(acc[j], r[j])], dtype=np.uint64) for j in (0, 1)]
    return acc[0], acc[1]


def bsgs_slots(params, v, baby, giant, d):
    """sum_i rot_{G_i}(sum_j d'_{i,j} * rot_{b_j}(v)) mod T on slot values, baby and giant as lists of (steps, swap)"""
    t = params[2]
    out = np.zeros(params[0], dtype=object)
    for (gs, gw), row in zip(giant, d):
        inner = np.zeros(params[0], dtype=object)
        for (bs, bw), dij in zip(baby, row):
            inner = (inner + np.asarray(dij, dtype=object) * np.asarray(rotate(v, bs, bw), dtype=object)) % t
        out = (out + np.asarray(rotate(inner, gs, gw), dtype=object)) % t
    return out.astype(np.uint64)


def steps_of(n, g):
    """(steps, swap) of the element g = 5^steps (2N - 1)^swap"""
    return next((k, sw) for sw in (False, True) for k in range(n // 2) if galois_element(n, k, sw) == g)


# ---- tests -------------------------------------------------------------------------------------------------------------------

def keys_of(params, s, elements, w, seed):
    keys = [ref_galois_key(params, s, seed, seed, g, w) for g in elements]
    return np.array([k[0] for k in keys]), np.array([k[1] for k in keys])


def test_restatement_is_the_composition_of_its_siblings():
    """the definition: bit-equal to ref_linear_transform per giant row, ref_hoisted_rotation of it, and a sum mod Q, at N = 16"""
    params, w = (16, Q60, 97, 19), 4
    n, q, t = params[0], params[1], params[2]
    s, pk0, pk1 = ref_keygen_share(params, b"\x74" * 32, b"\x74" * 32)
    rng = random.Random(5)
    c0, c1 = (np.array([rng.randrange(q) for _ in range(n)], dtype=np.uint64) for _ in range(2))
    g_baby = [1, galois_element(n, 1), galois_element(n, 1), galois_element(n, 2, True)]   # g = 1, a repeat, a swapped rotation
    g_giant = [galois_element(n, 4), 1, 2 * n - 1]
    bk0, bk1 = keys_of(params, s, g_baby, w, b"\x75" * 32)
    hk0, hk1 = keys_of(params, s, g_giant, w, b"\x76" * 32)
    diag = np.array([[circ([rng.randrange(-(t // 2), t // 2 + 1) for _ in range(n)], q) for _ in g_baby] for _ in g_giant])
    got = ref_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag)
    want = composed(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


DENSE = [((16, Q29, 97, 19), 4, nb) for nb in (1, 2, 4, 8)] + [((16, Q60, 97, 19), 4, nb) for nb in (1, 2, 4, 8)] + \
        [((16, Q60, 97, 19), 16, nb) for nb in (1, 2, 4, 8)] + [((64, Q60, 257, 19), 8, 8)]


@pytest.mark.parametrize("params,w,n_baby", DENSE)
def test_dense_matrix_decrypts_to_the_product(params, w, n_baby):
    n, q, t = params[0], params[1], params[2]
    s, pk0, pk1 = ref_keygen_share(params, b"\x71" * 32, b"\x71" * 32)
    rng = np.random.default_rng(n + w + n_baby)
    m = rng.integers(0, t, size=(n, n), dtype=np.uint64)
    v = rng.integers(0, t, size=n, dtype=np.uint64)
    c0, c1 = ref_encrypt(params, pk0, pk1, encode(params, v), b"\x72" * 32, 0)
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, m, n_baby)
    assert len(g_baby) == n_baby and len(g_giant) == 2 * -(-(n // 2) // n_baby) and d.shape == (len(g_giant), n_baby, n)
    bk0, bk1 = keys_of(params, s, g_baby, w, b"\x73" * 32)
    hk0, hk1 = keys_of(params, s, g_giant, w, b"\x77" * 32)
    diag = np.array([[encode(params, dij) for dij in row] for row in d])
    o0, o1 = ref_linear_transform_bsgs(params, c0, c1, g_baby, bk0, bk1, g_giant, hk0, hk1, w, diag)
    got = ref_decrypt(params, s, o0, o1)[0]
    noise, limit = ref_noise(params, s, o0, o1, got), q // t // 2
    print("dense N = %d, w = %d, n_baby = %d: noise 2^%.1f of 2^%.1f" % (n, w, n_baby, np.log2(max(noise, 1)), np.log2(limit)))
    want = (m.astype(object) @ v.astype(object) % t).astype(np.uint64)
    assert np.array_equal(eval_slots(params, got), want)
    assert noise < limit


def check_helper(params, m, n_baby, rng):
    n, t = params[0], params[2]
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, m, n_baby)
    assert d.shape == (len(g_giant), len(g_baby), n) and d.dtype == np.uint64
    baby, giant = [steps_of(n, g) for g in g_baby], [steps_of(n, g) for g in g_giant]
    v = rng.integers(0, t, size=n, dtype=np.uint64)
    want = (np.asarray(m).astype(object) % t @ v.astype(object) % t).astype(np.uint64)
    assert np.array_equal(bsgs_slots(params, v, baby, giant, d), want)
    return g_baby, g_giant, d, baby, giant


@pytest.mark.parametrize("n,n_babies", [(16, (None, 1, 3, 8)), (64, (None, 1, 5, 32))])
def test_helper_on_slot_values_small(n, n_babies):
    params, t = (n, Q60, 12289, 19), 12289
    rng = np.random.default_rng(n)
    m = rng.integers(0, t, size=(n, n), dtype=np.int64)
    half = n // 2
    for nb in n_babies:
        g_baby, g_giant, d, baby, giant = check_helper(params, m, nb, rng)
        nb = nb or 1 << -(-(n.bit_length() - 1) // 2)   # the default: 4 at N = 16, 8 at N = 64
        steps = -(-half // nb)
        assert g_baby == [galois_element(n, b) for b in range(nb)]
        assert g_giant == [galois_element(n, i * nb, sw) for sw in (False, True) for i in range(steps)]
        if half % nb:   # a non-divisor: the diagonals with k >= N/2 of the last giant step are zero
            assert not d[steps - 1, half - (steps - 1) * nb:].any() and not d[2 * steps - 1, half - (steps - 1) * nb:].any()


def test_helper_on_slot_values_at_1024():
    n, t = 1024, 12289
    params = (n, Q60, t, 19)
    rng = np.random.default_rng(1024)
    m = rng.integers(0, t, size=(n, n), dtype=np.int64)
    g_baby, g_giant, d, baby, giant = check_helper(params, m, None, rng)
    assert len(g_baby) == 32 and len(g_giant) == 32 and len(g_baby) + len(g_giant) - 2 == 62   # 62 keys: g = 1 needs none
    assert g_baby[0] == 1 and g_giant[0] == 1 and g_giant[16] == 2 * n - 1
    check_helper(params, m, 512, rng)
    check_helper(params, m, 1, rng)
    check_helper(params, m, 48, rng)   # a non-divisor of 512


def test_helper_drops_zero_rows_and_columns():
    n, t = 64, 257
    params = (n, Q60, t, 19)
    half, p = n // 2, np.arange(n)
    rng = np.random.default_rng(3)
    m = np.zeros((n, n), dtype=np.int64)
    for swap, offs in ((0, (0, 1, 17)), (1, (9,))):   # n_baby = 8: giant steps 0 and 2 unswapped, 1 swapped; baby columns 0 and 1
        for k in offs:
            m[p, ((p // half) ^ swap) * half + (p % half + k) % half] = rng.integers(1, t, size=n)
    g_baby, g_giant, d, baby, giant = check_helper(params, m, 8, rng)
    assert giant == [(0, False), (16, False), (8, True)] and baby == [(0, False), (1, False)]
    assert d.shape == (3, 2, n) and not d[1, 0].any() and not d[2, 0].any() and d[0, 0].all() and d[0, 1].all()
    # the stored diagonal is the diagonal rotated by the inverse of its giant step
    flat_g, flat_d = zk.bfv_matrix_diagonals(params, m)
    d17 = flat_d[flat_g.index(galois_element(n, 17))]
    assert np.array_equal(rotate(d[1, 1], 16), d17)
    d9s = flat_d[flat_g.index(galois_element(n, 9, True))]
    assert np.array_equal(rotate(d[2, 1], 8, True), d9s)
    g_baby, g_giant, d = zk.bfv_matrix_bsgs(params, np.zeros((n, n), dtype=np.int64))
    assert g_baby == [] and g_giant == [] and d.shape == (0, 0, n)
    with pytest.raises(ValueError):
        zk.bfv_matrix_bsgs(params, np.zeros((n, n + 1)))
    for bad in (0, half + 1):
        with pytest.raises(ValueError):
            zk.bfv_matrix_bsgs(params, m, bad)
    with pytest.raises(zk.ZkfheError, match="batching"):
        zk.bfv_matrix_bsgs((n, Q60, 7, 19), m)


def test_new_symbol_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    s = "zkfhe_bfv_linear_transform_bsgs"
    assert re.search(r"\bint %s\(" % s, header)
    assert s in zk.EXPORTS
    assert hasattr(lib, s)
    assert callable(zk.Context.bfv_linear_transform_bsgs)
    assert callable(zk.bfv_matrix_bsgs)
    assert zk.PROF_BFV_BSGS_INNER == 18 and zk.PROF_BFV_BSGS_GIANT == 19
    assert re.search(r"#define ZKFHE_PROF_BFV_BSGS_INNER 18\b", header) and re.search(r"#define ZKFHE_PROF_BFV_BSGS_GIANT 19\b", header)
    for word in ("already pre-rotated", "never needs a refusal", "neither read nor checked", "giant-major"):
        assert word in header, word
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "linear_transform_bsgs" in open(os.path.join(ROOT, doc)).read(), doc
