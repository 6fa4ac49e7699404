"""The bounds of zk-fhe_amd/csrc/fr9.hip.hpp (the nine-limb Fr value of the quotient, lookup, scan and batch-inversion kernels)
in exact Python integers: the product of tests/test_product_bounds_host.py (mont29, in the column order of mont29_c, peak |accumulator|
tracked) fed the LARGEST operands the static_asserts of fr9_mul, fr9_sqr and fr9_mul2 admit, and the operand types the kernels really
pass; the two loads and the register-level regrouping by five bits; the store over the whole range of a product's result.
No GPU, no compiler: tests/native/fr9_check.hip runs the C body on the same operands."""
import math
import random

import pytest

from oracle import pyref
from tests.test_product_bounds_host import INV_R, MASK, extreme, limbs_of, lz_weak, mont29, value

R = pyref.R
TOP = limbs_of(R)[8]


def result_v(vv):
    """Fr9P: a product of total bound vv returns |value| < 2 r (vv <= 160) or 3 r (vv <= 338)"""
    assert vv <= 338
    return 2 if vv <= 160 else 3


def check(pairs, bounds, sqr=False):
    """one product: the operands inside their types, the peak inside the signed accumulator, the result inside its type"""
    vv = 0
    for (a, b), ((la, ha, va), (lb, hb, vb)) in zip(pairs, bounds):
        for l, (lo, hi, v) in ((a, (la, ha, va)), (b, (lb, hb, vb))):
            assert all(-lo * (1 << 29) - (lo == 0) < x < hi * (1 << 29) + (hi == 0) for x in l[:8])
            assert abs(value(l)) < v * R and abs(l[8]) < 1 << 29 and v <= 127
        assert max(la, ha) * max(lb, hb) <= (2 if len(pairs) == 1 and not sqr else 1)
        vv += va * vb
    assert vv <= 338
    r, peak = mont29(pairs, R, INV_R, True, sqr)
    want = sum(value(a) * value(b) for a, b in pairs)
    assert abs(want) < 2 * (1 << 261) * R
    assert (value(r) << 261) % R == want % R
    assert all(0 <= v <= MASK for v in r[:8])
    k = result_v(vv)
    assert -(k - 1) * R < value(r) < k * R, value(r) / R
    assert abs(r[8]) < (k + 1) << 22
    assert peak < 1 << 63, "peak 2^%.3f" % math.log2(peak)
    return peak, value(r) / R


MUL_CASES = [   # (LO, HI, V) of both operands: the edges of the static_asserts, then what the kernels pass
    ((2, 2, 2), (1, 1, 127)), ((1, 1, 127), (2, 2, 2)), ((2, 2, 5), (0, 1, 66)), ((1, 2, 18), (1, 1, 18)), ((2, 1, 13), (1, 1, 26)),
    ((0, 2, 2), (0, 1, 64)),      # lookup term: (a + beta)(s + gamma)
    ((0, 1, 3), (0, 1, 66)),      # permutation step: running product x factor
    ((0, 1, 3), (0, 1, 32)),      # acc y
    ((0, 1, 2), (0, 1, 32)),      # inversion and scan chains
    ((0, 1, 1), (0, 1, 2)),       # sigma x beta in the 2^266 form
    ((0, 1, 32), (0, 1, 1)),      # fr9_cc
    ((0, 1, 32), (1, 1, 2)),      # l0 (1 - z0)
    ((1, 1, 64), (1, 1, 2)),      # (ap - apm)(ap - sp)
    ((0, 1, 1), (0, 1, 96)),      # against a regrouped product result
]


@pytest.mark.parametrize("sa", [False, True])
@pytest.mark.parametrize("sb", [False, True])
def test_fr9_mul_at_its_bounds(sa, sb):
    peaks = []
    for a, b in MUL_CASES:
        peaks.append(check([(extreme(*a, sa, R), extreme(*b, sb, R))], [(a, b)])[0])
    assert math.log2(max(peaks)) >= 61.5, "the operands do not reach the top: peak 2^%.3f" % math.log2(max(peaks))
    print("fr9_mul (signs %d %d): peak 2^%.3f" % (sa, sb, math.log2(max(peaks))))


MUL2_CASES = [
    ((0, 1, 3), (0, 1, 32), (0, 1, 32), (1, 1, 6)),       # Horner step of QG_PERM_D: acc y + lact (left - right)
    ((0, 1, 3), (0, 1, 32), (0, 1, 32), (0, 1, 4)),       # Horner step of a gate
    ((1, 1, 13), (1, 1, 13), (1, 1, 13), (1, 1, 13)),     # 338 exactly
    ((1, 1, 127), (1, 1, 1), (1, 1, 1), (1, 1, 127)),
    ((0, 1, 32), (0, 1, 2), (0, 1, 32), (1, 0, 2)),       # z1 A - z0 B
]


@pytest.mark.parametrize("sa", [False, True])
@pytest.mark.parametrize("sb", [False, True])
def test_fr9_mul2_at_its_bounds(sa, sb):
    peaks = []
    for a, b, c, d in MUL2_CASES:
        for flip in (False, True):   # the second product with the same sign (the terms add up) and with the opposite one (they cancel)
            pairs = [(extreme(*a, sa, R), extreme(*b, sb, R)), (extreme(*c, sa != flip, R), extreme(*d, sb, R))]
            peaks.append(check(pairs, [(a, b), (c, d)])[0])
    assert math.log2(max(peaks)) >= 61.5, "the operands do not reach the top: peak 2^%.3f" % math.log2(max(peaks))
    print("fr9_mul2 (signs %d %d): peak 2^%.3f" % (sa, sb, math.log2(max(peaks))))


@pytest.mark.parametrize("neg", [False, True])
def test_fr9_sqr_at_its_bound(neg):
    """limbs below 2^29 in magnitude, V^2 <= 338: V = 18"""
    x = extreme(1, 1, 18, neg, R)
    peak, ratio = check([(x, x)], [((1, 1, 18), (1, 1, 18))], sqr=True)
    assert mont29([(x, x)], R, INV_R, True, sqr=True)[0] == mont29([(x, x)], R, INV_R, True)[0]
    assert ratio >= 0
    print("fr9_sqr: peak 2^%.3f, result %.3f r" % (math.log2(peak), ratio))


def load32(w):
    """fr9_load32: limb i is bits [29 i - 5, 29 i + 24) of the packed word"""
    return [(w << 5) & MASK] + [(w >> (29 * i - 5)) & MASK for i in range(1, 9)]


def times32(l):
    """fr9_times32 on tight limbs with a signed top limb"""
    return [(l[0] << 5) & MASK] + [((l[i] << 5) & MASK) | (l[i - 1] >> 24) for i in range(1, 8)] + [l[8] * 32 + (l[7] >> 24)]


EDGES = [0, 1, R - 1, R - 2, 1 << 253, (1 << 253) - 1, value([MASK] * 8 + [TOP - 1]), (1 << 29) - 1, (1 << 232) - 1]


def test_loads_and_regrouping():
    rng = random.Random(9)
    for w in EDGES + [rng.randrange(R) for _ in range(200)]:
        c = load32(w)
        assert value(c) == 32 * w and all(0 <= x <= MASK for x in c) and value(c) < 32 * R
        assert times32(limbs_of(w)) == c
    # a product's result: (-2 r, 3 r), tight lower limbs -- the top limb of 32 x stays below 2^29
    for v in (3 * R - 1, 2 * R, R, 0, -1, -R, -2 * R + 1):
        l = [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]
        t = times32(l)
        assert value(t) == 32 * v and all(0 <= x <= MASK for x in t[:8]) and abs(t[8]) < 1 << 29


def test_store_over_a_products_range():
    """fr9_store is lz_weak and one conditional subtraction: every multiple of r in (-2 r, 3 r) and its neighbours, and the widest
    value a kernel stores or feeds a product as a difference (|v| < 6 r, limbs of either sign)"""
    for k in range(-6, 7):
        for d in (-1, 0, 1):
            v = k * R + d
            if abs(v) >= 6 * R:
                continue
            for lo, hi in ((0, 1), (1, 2)):
                l = [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]
                if lo:   # the same value with loose limbs: limb 1 lends 2^29 to limb 0, limb 2 borrows from limb 3
                    l[0] += 1 << 29
                    l[1] -= 1
                    l[2] -= 1 << 29
                    l[3] += 1
                w, q = lz_weak(l, lo, R)
                assert value(w) == v - q * R and 0 <= value(w) < 2 * R
                assert (value(w) - R if value(w) >= R else value(w)) == v % R
