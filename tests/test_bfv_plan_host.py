"""Host side of the prepared linear-transform plans (no GPU): the six zkfhe_bfv_plan_* symbols are declared, exported and mirrored,
and zkfhe_bfv_plan_bytes follows 4 (2 n_elems_total + 2 n_key_slots l N 5 + n_diagonals N 5) from zkfhe.h, at the header's worked
example and at both ends of N and of the digit width, and refuses what it says it refuses."""
import os
import re

import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, relin_digits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_plan_create", "zkfhe_bfv_plan_create_bsgs", "zkfhe_bfv_plan_apply", "zkfhe_bfv_plan_info", "zkfhe_bfv_plan_bytes",
               "zkfhe_bfv_plan_destroy"]


def formula(params, w, n_elems_total, n_key_slots, n_diagonals):
    n, l = params[0], relin_digits(params[1], w)
    return 4 * (2 * n_elems_total + 2 * n_key_slots * l * n * 5 + n_diagonals * n * 5)


def test_new_symbols_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    assert re.search(r"typedef struct zkfhe_bfv_plan zkfhe_bfv_plan;", header)
    assert callable(zk.bfv_plan_bytes)
    assert callable(zk.Context.bfv_plan) and callable(zk.Context.bfv_plan_bsgs)
    for method in ("apply", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(zk.BfvLinearPlan, method)), method
    for doc in ("INTEGRATION.md", "README.md"):
        assert "bfv_plan" in open(os.path.join(ROOT, doc)).read(), doc


def test_plan_bytes_of_the_dense_matrix():
    """the dense N = 1024 matrix of profiles/bfv_bsgs.md: 60-bit Q, w = 8 (l = 8), 32 x 32 elements, 62 key slots"""
    params = (1024, Q60, 12289, 19)
    assert relin_digits(Q60, 8) == 8
    assert 4 * 2 * 64 == 512 and 4 * 2 * 62 * 8 * 1024 * 5 == 20316160 and 4 * 1024 * 1024 * 5 == 20971520
    assert zk.bfv_plan_bytes(params, 8, 32 + 32, 62, 32 * 32) == 41288192


@pytest.mark.parametrize("params,w,l", [((8, Q29, 97, 19), 1, 29), ((32768, Q60, 65537, 19), 32, 2)])
def test_plan_bytes_follows_the_formula(params, w, l):
    assert relin_digits(params[1], w) == l == zk.bfv_relin_digits(params, w)
    for total, slots, diags in ((1, 0, 1), (1, 1, 1), (6, 4, 6), (64, 62, 1024), (7, 5, 12), ((1 << 20) - 1, (1 << 20) - 1, (1 << 20) - 1)):
        assert zk.bfv_plan_bytes(params, w, total, slots, diags) == formula(params, w, total, slots, diags), (total, slots, diags)
    assert zk.bfv_plan_bytes(params, w, 0, 0, 0) == 0


def test_plan_bytes_refusals():
    good = (1024, Q60, 12289, 19)
    for w in (0, -1, 33):
        with pytest.raises(zk.ZkfheError, match=r"bfv_plan_bytes: base_bits must be in \[1, 32\]"):
            zk.bfv_plan_bytes(good, w, 2, 1, 2)
    for bad in ((1000, Q60, 12289, 19), (4, Q60, 12289, 19), (65536, Q60, 12289, 19)):
        with pytest.raises(zk.ZkfheError, match="bfv params"):
            zk.bfv_plan_bytes(bad, 8, 2, 1, 2)
    lib = zk.load_library()
    assert lib.zkfhe_bfv_plan_bytes(None, 8, 2, 1, 2, None) != 0   # bytes is NULL
    assert "bfv_plan_bytes" in lib.zkfhe_last_error(None).decode()
    assert lib.zkfhe_bfv_plan_info(None, None, None, None, None) != 0   # plan is NULL
    assert "bfv_plan_info" in lib.zkfhe_last_error(None).decode()
    assert lib.zkfhe_bfv_plan_destroy(None, None) == 0   # nothing to free
