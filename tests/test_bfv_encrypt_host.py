"""Host side of GPU BFV encryption (no GPU): the error sampler's table against an exact computation of the truncated discrete
Gaussian, parameter checks, and the declarations / exports of the new entry points."""
import decimal
import os
import re

import pytest

import zk_fhe_amd as zk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_poly_mul_ternary_negacyclic", "zkfhe_bfv_error_cdt", "zkfhe_bfv_fhe_keypair", "zkfhe_bfv_encrypt",
               "zkfhe_bfv_decrypt", "zkfhe_bfv_prove_words"]


def exact_cdt(b, sigma="3.2"):
    """2^64 P(X <= -B + i), i < 2 B, for X the discrete Gaussian of width sigma restricted to [-B, B], at 60 digits"""
    ctx = decimal.Context(prec=60)
    s2 = 2 * decimal.Decimal(sigma) ** 2
    w = [ctx.exp(-decimal.Decimal(x * x) / s2) for x in range(-b, b + 1)]
    z = ctx.add(decimal.Decimal(0), sum(w, decimal.Decimal(0)))
    out, acc = [], decimal.Decimal(0)
    for i in range(2 * b):
        acc = ctx.add(acc, w[i])
        out.append(ctx.multiply(ctx.divide(acc, z), decimal.Decimal(2) ** 64))
    return out


@pytest.mark.parametrize("b", [1, 19, 100])
def test_error_table_matches_exact_cdf(b):
    got = zk.bfv_error_cdt((1024, 536870909, 7, b))
    assert len(got) == 2 * b
    want = exact_cdt(b)
    tol = decimal.Decimal(2) ** 16   # 2^-48 of 2^64
    for i, (g, w) in enumerate(zip(got, want)):
        assert abs(decimal.Decimal(int(g)) - w) <= tol, (b, i, int(g), w)


@pytest.mark.parametrize("b", [1, 19, 100, 1023])
def test_error_table_is_monotone(b):
    got = [int(x) for x in zk.bfv_error_cdt((1024, (1 << 60) - 93, 65537, b))]
    assert all(x <= y for x, y in zip(got, got[1:]))
    assert got[-1] < 1 << 64
    # symmetric around zero, P(X <= -B + i) + P(X <= B - 1 - i) = 1, well inside the 2^-48 budget
    for i in range(2 * b):
        assert abs(got[i] + got[2 * b - 1 - i] - (1 << 64)) <= 1 << 8


@pytest.mark.parametrize("params", [
    (1000, 536870909, 7, 19),        # N not a power of two
    (4, 536870909, 7, 19),           # N < 8
    (65536, 536870909, 7, 19),       # N > 32768
    (1024, 1, 1, 1),                 # Q < 2
    (1024, 1 << 63, 7, 19),          # Q >= 2^63
    (1024, 536870909, 1, 19),        # T < 2
    (1024, 536870909, 536870909, 19),  # T >= Q
    (1024, 536870909, 7, 0),         # B < 1
    (1024, 536870909, 7, 1024),      # B >= 1024
    (1024, 17, 7, 17),               # B >= Q
])
def test_out_of_range_parameters_are_refused(params):
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        zk.bfv_error_cdt(params)


def test_boundary_parameters_are_accepted():
    assert len(zk.bfv_error_cdt((8, 3, 2, 1))) == 2
    assert len(zk.bfv_error_cdt((32768, (1 << 63) - 1, (1 << 63) - 2, 1023))) == 2046


def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    assert "zkfhe_bfv_words" in header
    for name in ("poly_mul_ternary_negacyclic", "bfv_fhe_keypair", "bfv_encrypt", "bfv_decrypt"):
        assert callable(getattr(zk.Context, name))
    assert callable(zk.BfvProvingKey.prove_words) and callable(zk.BfvProvingKey.encrypt_and_prove)
