"""Host side of GPU BFV evaluation (no GPU): the declarations and exports of the new entry points, the relinearization digit count,
and the exact negacyclic product that the GPU tests use as their oracle (Kronecker substitution on Python integers) against a
schoolbook sum.  The oracle helpers here restate the definitions of zkfhe.h; tests/test_gpu_bfv_eval.py imports them."""
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_add", "zkfhe_bfv_sum", "zkfhe_bfv_add_plain", "zkfhe_bfv_mul_plain", "zkfhe_bfv_relin_digits",
               "zkfhe_bfv_relin_keygen", "zkfhe_bfv_mul", "zkfhe_bfv_noise"]
Q29, Q60, Q63 = 536870909, (1 << 60) - 93, (1 << 63) - 25


# ---- the oracle --------------------------------------------------------------------------------------------------------------

def kron_negacyclic(pairs, n):
    """sum of a * b over `pairs` exactly in Z[x]/(x^N + 1): coefficient lists in degree order, signed Python integers.  Kronecker
    substitution: each polynomial is packed into one integer with W-bit slots (every value offset by 2^(W-1) so that the slots are
    non-negative), the integers are multiplied, and the slots of the offset product are read back."""
    bound = 1
    for a, b in pairs:
        bound += n * max(1, max(abs(int(x)) for x in a)) * max(1, max(abs(int(x)) for x in b))
    W = (bound.bit_length() + 2 + 7) // 8 * 8
    nb, off = W // 8, 1 << (W - 1)

    def ones(count):
        return int.from_bytes((b"\x01" + b"\x00" * (nb - 1)) * count, "little")

    def pack(v):
        return int.from_bytes(b"".join((int(x) + off).to_bytes(nb, "little") for x in v), "little") - off * ones(len(v))

    total = sum(pack(a) * pack(b) for a, b in pairs)
    raw = (total + off * ones(2 * n)).to_bytes(2 * n * nb, "little")
    full = [int.from_bytes(raw[i * nb:(i + 1) * nb], "little") - off for i in range(2 * n)]
    return [full[k] - full[k + n] for k in range(n)]


def schoolbook_negacyclic(a, b):
    n = len(a)
    out = [0] * n
    for i in range(n):
        for j in range(n):
            k = i + j
            if k < n:
                out[k] += a[i] * b[j]
            else:
                out[k - n] -= a[i] * b[j]
    return out


def centred(v, q):
    """residues (any order) -> signed integers, v - Q above floor(Q/2)"""
    return [int(x) - q if int(x) > q // 2 else int(x) for x in v]


def deg(v):
    """CircuitInput order (highest degree first) -> degree order, as Python integers"""
    return [int(x) for x in np.asarray(v)[::-1]]


def circ(v, q):
    """degree order -> CircuitInput order, residues mod Q"""
    return np.array([int(x) % q for x in v[::-1]], dtype=np.uint64)


def relin_digits(q, w):
    return -(-(q - 1).bit_length() // w)


def ref_tensor(params, a0, a1, b0, b1):
    """c^_0, c^_1, c^_2 of zkfhe_bfv_mul in degree order: floor((2 T x_j + Q) / 2Q) mod Q of the exact products of the centred inputs"""
    n, q, t = params[0], params[1], params[2]
    A0, A1, B0, B1 = (centred(deg(x), q) for x in (a0, a1, b0, b1))
    xs = (kron_negacyclic([(A0, B0)], n), kron_negacyclic([(A0, B1), (A1, B0)], n), kron_negacyclic([(A1, B1)], n))
    return [[(2 * t * x + q) // (2 * q) % q for x in xj] for xj in xs]


def ref_mul(params, a0, a1, b0, b1, rlk0, rlk1, w):
    """zkfhe_bfv_mul of one pair, restated from its definition (zkfhe.h); CircuitInput order in and out"""
    n, q = params[0], params[1]
    c0, c1, c2 = ref_tensor(params, a0, a1, b0, b1)
    l = relin_digits(q, w)
    digits = [[(c >> (i * w)) & ((1 << w) - 1) for c in c2] for i in range(l)]
    s0 = kron_negacyclic([(digits[i], deg(rlk0[i])) for i in range(l)], n)
    s1 = kron_negacyclic([(digits[i], deg(rlk1[i])) for i in range(l)], n)
    return circ([x + y for x, y in zip(c0, s0)], q), circ([x + y for x, y in zip(c1, s1)], q)


# ---- tests -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 8, 16, 33])
def test_kronecker_matches_schoolbook(n):
    rng = random.Random(n)
    for bits in (3, 62, 140):
        a = [rng.randrange(-(1 << bits), 1 << bits) for _ in range(n)]
        b = [rng.randrange(-(1 << bits), 1 << bits) for _ in range(n)]
        c = [rng.randrange(-(1 << bits), 1 << bits) for _ in range(n)]
        assert kron_negacyclic([(a, b)], n) == schoolbook_negacyclic(a, b)
        want = [x + y for x, y in zip(schoolbook_negacyclic(a, b), schoolbook_negacyclic(c, a))]
        assert kron_negacyclic([(a, b), (c, a)], n) == want


def test_kronecker_extremes():
    n, v = 16, (Q63 // 2)
    for sa, sb in ((1, 1), (1, -1), (-1, -1)):
        a, b = [sa * v] * n, [sb * v] * n
        got = kron_negacyclic([(a, b), (b, a)], n)
        assert got == [2 * x for x in schoolbook_negacyclic(a, b)]
        assert got == [2 * sa * sb * v * v * (2 * k + 2 - n) for k in range(n)]
    assert kron_negacyclic([([0] * 8, [5] * 8)], 8) == [0] * 8


def test_reference_mul_small_case():
    # the definition on a hand-sized case: N = 8, Q = 97, T = 5, w = 3
    params, w = (8, 97, 5, 1), 3
    rng = random.Random(7)
    pick = lambda: np.array([rng.randrange(97) for _ in range(8)], dtype=np.uint64)  # noqa: E731
    a0, a1, b0, b1 = pick(), pick(), pick(), pick()
    l = relin_digits(97, w)
    assert l == 3
    rlk0 = np.array([pick() for _ in range(l)])
    rlk1 = np.array([pick() for _ in range(l)])
    out0, out1 = ref_mul(params, a0, a1, b0, b1, rlk0, rlk1, w)
    A0, A1, B0, B1 = (centred(deg(x), 97) for x in (a0, a1, b0, b1))
    x2 = schoolbook_negacyclic(A1, B1)
    c2 = [(2 * 5 * x + 97) // 194 % 97 for x in x2]
    x0 = schoolbook_negacyclic(A0, B0)
    c0 = [(2 * 5 * x + 97) // 194 % 97 for x in x0]
    acc = [0] * 8
    for i in range(l):
        d = [(c >> (3 * i)) & 7 for c in c2]
        acc = [x + y for x, y in zip(acc, schoolbook_negacyclic(d, deg(rlk0[i])))]
    assert list(out0) == [int(x) for x in circ([x + y for x, y in zip(c0, acc)], 97)]
    assert out1.dtype == np.uint64 and out1.shape == (8,)


@pytest.mark.parametrize("q", [3, 97, Q29, Q60, Q63, (1 << 62) + 1])
def test_relin_digits(q):
    for w in range(1, 33):
        assert zk.bfv_relin_digits((8, q, 2, 1), w) == relin_digits(q, w), (q, w)


def test_relin_digits_refuses_base_bits():
    for w in (0, -1, 33, 64):
        with pytest.raises(zk.ZkfheError, match=r"base_bits must be in \[1, 32\]"):
            zk.bfv_relin_digits((1024, Q60, 65537, 19), w)
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        zk.bfv_relin_digits((1000, Q60, 65537, 19), 16)


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    for name in ("bfv_add", "bfv_sum", "bfv_add_plain", "bfv_mul_plain", "bfv_relin_keygen", "bfv_mul", "bfv_noise"):
        assert callable(getattr(zk.Context, name)), name
    assert callable(zk.bfv_relin_digits)
