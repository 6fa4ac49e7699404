"""Host side of ring packing (no GPU): pure-Python restatements of the monomial product, the scaling by N^-1, the pack elements and
the pack of zkfhe.h "Ring packing" in its level form, built from ref_apply_galois, add and neg of the existing host tests.  At three
small shapes and every n in {1, 2, 3, 5, N/2, N - 1, N} with random positions the restated pack decrypts to the chosen coefficients
at i N / n' and zero elsewhere, equals the recursive even/odd formulation bit for bit, and its noise is within the header's bound,
which at these shapes is itself below floor(Q/T)/2: decryption is guaranteed, not lucky.  Also the host-only call against the
restatement, the declarations and exports, and the refusals that need no device.  tests/test_gpu_bfv_pack.py imports the
restatements."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, circ, deg, relin_digits
from tests.test_bfv_galois_host import ref_apply_galois, ref_galois_key
from tests.test_bfv_threshold_host import add, neg, ref_decrypt, ref_encrypt, ref_keygen_share, ref_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_pack_elements", "zkfhe_bfv_mul_monomial", "zkfhe_bfv_pack", "zkfhe_bfv_cts_mul_monomial", "zkfhe_bfv_cts_pack"]
SHAPES = [((8, Q29, 7, 19), 8), ((16, Q60, 97, 19), 16), ((32, Q29, 7, 19), 4)]
KEY_SEED, ENC_SEED, GK_SEED = b"\x61" * 32, b"\x62" * 32, b"\x63" * 32


# ---- the definitions, restated from zkfhe.h --------------------------------------------------------------------------------

def monomial(v, k, q):
    """x^k v mod (x^N + 1, Q) for 0 <= k < 2N: coefficient i moves to j = i + k mod 2N, negated and placed at j - N past N"""
    d = deg(v)
    n = len(d)
    assert 0 <= k < 2 * n
    out = [0] * n
    for i, x in enumerate(d):
        j = (i + k) % (2 * n)
        if j < n:
            out[j] = x
        else:
            out[j - n] = -x
    return circ(out, q)


def scale(v, q):
    """every coefficient times nu = N^-1 mod Q"""
    nu = pow(len(v), -1, q)
    return np.array([int(x) * nu % q for x in v], dtype=np.uint64)


def pack_elements(n):
    return [(1 << l) + 1 for l in range(1, n.bit_length())]


def sub(a, b, q):
    return add(a, neg(b, q), q=q)


def padded(n):
    """n', the least power of two >= n"""
    return 1 << (n - 1).bit_length()


def prepare(params, c0, c1, pos):
    """step 1: w_i = nu x^((2N - pos_i) mod 2N) a_i, then zeros up to n'"""
    n_ring, q = params[0], params[1]
    w = [tuple(scale(monomial(c, (2 * n_ring - int(p)) % (2 * n_ring), q), q) for c in (c0[i], c1[i])) for i, p in enumerate(pos)]
    zero = np.zeros(n_ring, dtype=np.uint64)
    return w + [(zero, zero)] * (padded(len(w)) - len(w))


def pack_step(params, e, o, lv, gk0, gk1, w):
    """one pair of level lv: (e + t) + apply_galois(e - t, 2^lv + 1) with t = x^(N / 2^lv) o; o None: a trace level"""
    n_ring, q = params[0], params[1]
    g = (1 << lv) + 1
    if o is None:
        total, diff = e, e
    else:
        t = [monomial(c, n_ring >> lv, q) for c in o]
        total, diff = [add(a, b, q=q) for a, b in zip(e, t)], [sub(a, b, q) for a, b in zip(e, t)]
    k0, k1 = ref_apply_galois(params, diff[0], diff[1], g, gk0[lv - 1], gk1[lv - 1], w)
    return add(total[0], k0, q=q), add(total[1], k1, q=q)


def ref_pack(params, c0, c1, pos, gk0, gk1, w):
    """zkfhe_bfv_pack of one group restated in the level form: c0, c1 of shape (n, N), pos n positions (None: all 0), gk0, gk1 the
    keys of pack_elements in order"""
    n_ring = params[0]
    log_n = n_ring.bit_length() - 1
    wi = prepare(params, c0, c1, [0] * len(c0) if pos is None else pos)
    levels = len(wi).bit_length() - 1
    for lv in range(1, levels + 1):
        h = len(wi) >> 1
        wi = [pack_step(params, wi[i], wi[i + h], lv, gk0, gk1, w) for i in range(h)]
    for lv in range(levels + 1, log_n + 1):
        wi = [pack_step(params, wi[0], None, lv, gk0, gk1, w)]
    return wi[0]


def ref_pack_recursive(params, c0, c1, pos, gk0, gk1, w):
    """PackLWEs in its even/odd form followed by the trace: pack(list) = (E + x^(N/len) O) + sigma_(len+1)(E - x^(N/len) O) with E,
    O the packs of the even- and odd-indexed halves"""
    n_ring = params[0]
    log_n = n_ring.bit_length() - 1

    def rec(ws):
        if len(ws) == 1:
            return ws[0]
        return pack_step(params, rec(ws[0::2]), rec(ws[1::2]), log_n - (n_ring // len(ws)).bit_length() + 1, gk0, gk1, w)

    # the innermost pairs of the even/odd tree differ in the highest bit of their index: i and i + n'/2, the pairs of level 1
    wi = prepare(params, c0, c1, [0] * len(c0) if pos is None else pos)
    out = rec(wi)
    for lv in range(len(wi).bit_length(), log_n + 1):
        out = pack_step(params, out, None, lv, gk0, gk1, w)
    return out


def expected_plain(params, ms, pos):
    """the plaintext a pack decrypts to: coefficient i N / n' is coefficient pos_i of m_i, everything else 0"""
    n_ring = params[0]
    step = n_ring // padded(len(ms))
    out = [0] * n_ring
    for i, m in enumerate(ms):
        out[i * step] = deg(m)[0 if pos is None else int(pos[i])]
    return np.array(out[::-1], dtype=np.uint64)


def noise_bound(params, w, input_noise):
    """the header's sufficient bound: max_i noise(a_i) + (N - 1) l N (2^w - 1) B"""
    n_ring, q, b = params[0], params[1], params[3]
    return input_noise + (n_ring - 1) * relin_digits(q, w) * n_ring * ((1 << w) - 1) * b


def plain(rng, params):
    n_ring, q, t = params[0], params[1], params[2]
    return np.array([rng.randrange(-(t // 2), t // 2 + 1) % q for _ in range(n_ring)], dtype=np.uint64)


def pack_keys(params, s, w, crs=GK_SEED, party=GK_SEED):
    keys = [ref_galois_key(params, s, crs, party, g, w) for g in pack_elements(params[0])]
    return np.array([k[0] for k in keys]), np.array([k[1] for k in keys])


def list_of_n(n_ring):
    return sorted({1, 2, 3, 5, n_ring // 2, n_ring - 1, n_ring})


# ---- tests -------------------------------------------------------------------------------------------------------------------

def test_monomial_and_scale_restated():
    q = Q29
    v = np.array([3, q - 1, 0, 5, 7, 11, q - 2, 1], dtype=np.uint64)
    n = len(v)
    assert np.array_equal(monomial(v, 0, q), v)
    assert np.array_equal(monomial(v, n, q), neg(v, q))
    assert np.array_equal(monomial(monomial(v, 3, q), 2 * n - 3, q), v)
    assert np.array_equal(monomial(monomial(v, n - 1, q), 2, q), monomial(v, n + 1, q))
    one = circ([1] + [0] * (n - 1), q)
    assert deg(monomial(one, 1, q)) == [0, 1] + [0] * (n - 2) and deg(monomial(one, 2 * n - 1, q)) == [0] * (n - 1) + [q - 1]
    assert np.array_equal(np.array([int(x) * n % q for x in scale(v, q)], dtype=np.uint64), v)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "N%d-w%d" % (s[0][0], s[1]))
def shape(request):
    """the keys, 2 N fresh encryptions and their noise at one shape, made once"""
    params, w = request.param
    n_ring = params[0]
    rng = random.Random(n_ring * 100 + w)
    s, pk0, pk1 = ref_keygen_share(params, KEY_SEED, KEY_SEED)
    gk0, gk1 = pack_keys(params, s, w)
    ms = [plain(rng, params) for _ in range(n_ring)]
    cts = [ref_encrypt(params, pk0, pk1, m, ENC_SEED, i) for i, m in enumerate(ms)]
    fresh = max(ref_noise(params, s, c[0], c[1], m) for c, m in zip(cts, ms))
    return params, w, s, gk0, gk1, ms, cts, fresh, rng


def test_the_bound_guarantees_decryption_at_these_shapes(shape):
    params, w, _, _, _, _, _, fresh, _ = shape
    q, t = params[1], params[2]
    assert noise_bound(params, w, fresh) < (q // t) // 2


def test_restated_pack_decrypts_matches_the_recursion_and_keeps_the_bound(shape):
    params, w, s, gk0, gk1, ms, cts, fresh, rng = shape
    n_ring = params[0]
    for n in list_of_n(n_ring):
        pos = [rng.randrange(n_ring) for _ in range(n)]
        c0, c1 = [c[0] for c in cts[:n]], [c[1] for c in cts[:n]]
        o0, o1 = ref_pack(params, c0, c1, pos, gk0, gk1, w)
        want = expected_plain(params, ms[:n], pos)
        assert np.array_equal(ref_decrypt(params, s, o0, o1)[0], want), n
        r0, r1 = ref_pack_recursive(params, c0, c1, pos, gk0, gk1, w)
        assert np.array_equal(o0, r0) and np.array_equal(o1, r1), n
        assert ref_noise(params, s, o0, o1, want) <= noise_bound(params, w, fresh), n
    o0, o1 = ref_pack(params, [cts[0][0], cts[1][0]], [cts[0][1], cts[1][1]], None, gk0, gk1, w)
    assert np.array_equal(ref_decrypt(params, s, o0, o1)[0], expected_plain(params, ms[:2], None))


def test_pack_elements_match_the_restatement():
    for log_n in range(3, 16):
        n_ring = 1 << log_n
        got = zk.bfv_pack_elements((n_ring, Q60, 65537, 19))
        assert got == pack_elements(n_ring) and len(got) == log_n and got[0] == 3 and got[-1] == n_ring + 1
    assert zk.bfv_pack_elements((8, Q29, 7, 19)) == [3, 5, 9]          # a T that does not batch
    assert zk.bfv_pack_elements((1024, Q29, 7, 19)) == pack_elements(1024)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        zk.bfv_pack_elements((12, Q29, 7, 19))


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    assert re.search(r"#define ZKFHE_PROF_BFV_PACK 27\b", header) and zk.PROF_BFV_PACK == 27
    for word in ("Ring packing", "nu = N^-1 mod Q", "Q must be odd", "(N - 1) l_digits N (2^w - 1) B"):
        assert word in header, word


def test_python_methods_exist():
    assert callable(zk.bfv_pack_elements)
    for name in ("bfv_mul_monomial", "bfv_pack"):
        assert callable(getattr(zk.Context, name)), name
    for name in ("mul_monomial", "pack"):
        assert callable(getattr(zk.BfvCiphertexts, name)), name


def test_calls_without_a_context_are_refused_before_any_device_work():
    lib = zk.load_library()
    prm = zk.BfvParamsC(8, Q29, 7, 19)
    cases = [("zkfhe_bfv_mul_monomial", "bfv_mul_monomial", [None, ctypes.byref(prm), 1, None, None, 1, None, None, None]),
             ("zkfhe_bfv_pack", "bfv_pack", [None, ctypes.byref(prm), 1, 1, None, None, None, None, None, 8, None, None]),
             ("zkfhe_bfv_cts_mul_monomial", "bfv_cts_mul_monomial", [None, None, 1, None, None]),
             ("zkfhe_bfv_cts_pack", "bfv_cts_pack", [None, None, 1, None, None, None])]
    for symbol, name, args in cases:
        f = getattr(lib, symbol)
        assert f(*args) != 0, name
        assert lib.zkfhe_last_error(None).decode() == "%s: a NULL argument or a zero count" % name
    g = lib.zkfhe_bfv_pack_elements
    assert g(ctypes.byref(prm), None, None) != 0
    assert lib.zkfhe_last_error(None).decode() == "bfv_pack_elements: count is NULL"
