"""Host side of the BFV edge tests (no GPU): the tie enumeration that tests/test_gpu_bfv_edges.py rounds at, checked against exact
rational rounding; the relinearization digit count at every power of two; and the error table at its smallest and largest B.
The helpers here are imported by the GPU file."""
import math
import random
from fractions import Fraction

import pytest

import zk_fhe_amd as zk
from tests.test_bfv_encrypt_host import exact_cdt
from tests.test_bfv_eval_host import Q29, Q60, Q63, relin_digits

Q62 = 1 << 62                 # a power of two: delta = Q / T is exact for T = 2^k
QE = 2 * ((1 << 61) - 1)      # even, not a power of two (twice the Mersenne prime 2^61 - 1)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------

def round_q(x, q, t):
    """round(T x / Q) with ties rounded up, on Python integers: floor((2 T x + Q) / 2Q) (zkfhe_bfv_mul's c^_j, inputs.decrypt)"""
    return (2 * t * x + q) // (2 * q)


def decrypt_value(x, q, t):
    """the decryption of one coefficient of [c0 + c1 s]_Q (any representative x): round(T x / Q) mod T, centred, as a residue mod Q"""
    x = int(x) % q
    x = x - q if x > q // 2 else x
    r = round_q(x, q, t) % t
    return (r - t if r > t // 2 else r) % q


def tie_values(q, t, c=1, per_class=2):
    """(a, r) with a in [-floor(Q/2), floor(Q/2)] and 2 T |c a| + Q = r (mod 2Q) for r in {0, 1, -1}: the products c a at which
    round(T c a / Q) is an exact tie (r = 0, which needs even Q) or one step from one.  Both signs of a; of each class the first and
    last `per_class` solutions in [0, floor(Q/2)]."""
    A = 2 * t * abs(c) % (2 * q)
    out = []
    if A == 0:
        return out
    g = math.gcd(A, 2 * q)
    M = 2 * q // g
    for r in (0, 1, -1):
        target = (q + r) % (2 * q)   # 2 T |c| a = r - Q = r + Q (mod 2Q)
        if target % g:
            continue
        a0 = (target // g) * pow(A // g, -1, M) % M if M > 1 else 0
        if a0 > q // 2:
            continue
        count = (q // 2 - a0) // M + 1
        for k in sorted(set(range(min(per_class, count))) | set(range(max(0, count - per_class), count))):
            a = a0 + k * M
            out.append((a, r))
            if a:
                out.append((-a, r))
    return out


def tie_class(x, q, t):
    """r in {0, 1, -1} with 2 T |x| + Q = r (mod 2Q), else None"""
    v = (2 * t * abs(x) + q) % (2 * q)
    return {0: 0, 1: 1, 2 * q - 1: -1}.get(v)


# the (Q, T) pairs of the rounding tests: odd Q, a power of two, even Q; T even and odd, small and near Q
TIE_PARAMS = [(Q63, 1 << 20), (Q63, 65537), (Q62, 1 << 20), (Q62, 3 ** 13), (QE, 65537), (QE, 1 << 20), (Q60, Q60 - 2),
              (Q62, Q62 - 1), (4, 2), (3, 2), (97, 5), (96, 6)]


# ---- tests -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q,t", TIE_PARAMS)
def test_tie_values_are_ties(q, t):
    rng = random.Random(q ^ t)
    for c in (1, -1, 3, q // 2, -(q // 2), q // 2 - 1, rng.randrange(1, q // 2 + 1) | 1):
        ties = tie_values(q, t, c)
        for a, r in ties:
            assert abs(a) <= q // 2
            x = c * a
            assert tie_class(x, q, t) == r, (c, a)
            frac = Fraction(t * x, q) - math.floor(Fraction(t * x, q))
            if r == 0:
                assert frac == Fraction(1, 2), (c, a)
            else:   # one 2Q-th away from the tie, on either side
                assert abs(frac - Fraction(1, 2)) == Fraction(1, 2 * q), (c, a)
            assert round_q(x, q, t) == math.floor(Fraction(t * x, q) + Fraction(1, 2))
        if c == 1 and q % 2 == 0 and t % 2 == 1:   # T Q/2 / Q = T/2: Q/2 itself is a tie
            assert (q // 2, 0) in ties
    # and away from ties
    for x in [0, 1, -1, q // 2, -(q // 2), q - 1, 1 - q] + [rng.randrange(-(1 << 140), 1 << 140) for _ in range(200)]:
        assert round_q(x, q, t) == math.floor(Fraction(t * x, q) + Fraction(1, 2)), x


def test_tie_values_reach_exact_ties_where_they_exist():
    # the exact class needs even Q; with Q = 2^62 and T = 2^20 it is a = 2^41 (mod 2^42), for every odd multiplier
    for c in (1, -1, 3, (1 << 61) - 1):
        exact = [a for a, r in tie_values(Q62, 1 << 20, c) if r == 0]
        assert exact and all(abs(a) % (1 << 42) == 1 << 41 for a in exact), c
        assert any(a < 0 for a in exact) and any(a > 0 for a in exact)
    assert all(r != 0 for _, r in tie_values(Q63, 1 << 20)) and tie_values(Q63, 1 << 20)   # odd Q: near ties only
    assert [a for a, r in tie_values(QE, 65537) if r == 0]


@pytest.mark.parametrize("q,t", TIE_PARAMS)
def test_decrypt_value_matches_rational_rounding(q, t):
    rng = random.Random(q + t)
    xs = [a for a, _ in tie_values(q, t)] + [0, 1, -1, q // 2, q // 2 + 1, q - 1] + [rng.randrange(q) for _ in range(100)]
    for x in xs:
        xc = x % q
        xc = xc - q if xc > q // 2 else xc
        m = math.floor(Fraction(t * xc, q) + Fraction(1, 2)) % t
        m = m - t if m > t // 2 else m
        assert decrypt_value(x, q, t) == m % q, x


def test_relin_digits_at_powers_of_two():
    for k in range(2, 63):
        q = 1 << k
        assert (q - 1).bit_length() == k
        for w in range(1, 33):
            want = -(-k // w)
            assert relin_digits(q, w) == want
            assert zk.bfv_relin_digits((8, q, 2, 1), w) == want, (k, w)
        for qq in (q - 1, q + 1):   # the neighbours: bitlen(Q - 1) = k - 1 or k
            if qq >= 3 and qq < 1 << 63:
                for w in (1, 2, 7, 31, 32):
                    assert zk.bfv_relin_digits((8, qq, 2, 1), w) == relin_digits(qq, w), (qq, w)
    for q in (Q29, Q60, Q63, (1 << 63) - 1):
        for w in range(1, 33):
            assert zk.bfv_relin_digits((8, q, 2, 1), w) == relin_digits(q, w), (q, w)


@pytest.mark.parametrize("b", [2, 1023])
def test_error_table_exact_at_the_ends(b):
    got = zk.bfv_error_cdt((1024, Q60, 65537, b))
    assert len(got) == 2 * b
    want = exact_cdt(b)
    tol = 1 << 16   # 2^-48 of 2^64, as test_error_table_matches_exact_cdf
    for i, (g, w) in enumerate(zip(got, want)):
        assert abs(int(g) - w) <= tol, (b, i, int(g), w)
    if b == 1023:   # the far tails are below 2^-64: the table starts at 0 and ends at 2^64 - 1
        assert int(got[0]) == 0 and int(got[-1]) == (1 << 64) - 1
