"""Resident evaluation keys without a GPU (bfv_evk.hip): the new entry points are exported and declared, the host-only calls answer,
and the Python object refuses to exist without a context."""
import ctypes
import os
import re

import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zkfhe_bfv_evk_create", "zkfhe_bfv_evk_bytes", "zkfhe_bfv_evk_info", "zkfhe_bfv_evk_destroy", "zkfhe_bfv_evk_wide_max",
         "zkfhe_bfv_cts_mul_evk", "zkfhe_bfv_cts_apply_galois_evk", "zkfhe_bfv_cts_slot_sum", "zkfhe_bfv_cts_dot", "zkfhe_bfv_cts_dot_plain"]


def test_names_are_exported_and_declared():
    lib = zk.load_library()
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    for name in NAMES:
        assert name in zk.EXPORTS, name
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"#define ZKFHE_PROF_BFV_KEY_SWITCH_WIDE 26\b", header) and zk.PROF_BFV_KEY_SWITCH_WIDE == 26
    assert re.search(r"#define ZKFHE_PROF_BFV_RESIDENT 25\b", header) and zk.PROF_BFV_RESIDENT == 25


@pytest.mark.parametrize("params,w,l", [((8, Q29, 7, 19), 8, 4), ((1024, Q29, 7, 19), 32, 1), ((4096, Q60, 65537, 19), 16, 4)])
def test_bytes_is_the_formula(params, w, l):
    assert zk.bfv_relin_digits(params, w) == l
    for has_relin, n_galois in [(1, 0), (0, 1), (1, 3), (0, 15)]:
        assert zk.bfv_evk_bytes(params, w, has_relin, n_galois) == (has_relin + n_galois) * 2 * l * 5 * params[0] * 4
    with pytest.raises(zk.ZkfheError, match="bfv_evk_bytes: base_bits"):
        zk.bfv_evk_bytes(params, 0, 1, 0)


def test_info_of_null_is_refused():
    lib = zk.load_library()
    f = lib.zkfhe_bfv_evk_info
    assert f(None, None, None, None, None, None, None) != 0
    assert lib.zkfhe_last_error(None).decode() == "bfv_evk_info: evk is NULL"


def test_destroy_of_null_is_not_an_error():
    lib = zk.load_library()
    f = lib.zkfhe_bfv_evk_destroy
    assert f(None, None) == 0


def test_calls_without_a_context_are_refused_before_any_device_work():
    lib = zk.load_library()
    prm = zk.BfvParamsC(8, Q29, 7, 1)
    out = ctypes.c_void_p(1)
    f = lib.zkfhe_bfv_evk_create
    assert f(None, ctypes.byref(prm), 8, None, None, 0, None, None, None, ctypes.byref(out)) != 0 and not out.value
    assert lib.zkfhe_last_error(None).decode() == "bfv_evk_create: a NULL argument or a zero count"
    for name, args in [("mul_evk", [None] * 5), ("apply_galois_evk", [None, None, 5, None, None]), ("slot_sum", [None] * 4),
                       ("dot", [None, None, None, 1, None, None]), ("dot_plain", [None, None, 1, 1, None, None])]:
        g = getattr(lib, "zkfhe_bfv_cts_" + name)
        assert g(*args) != 0, name
        assert lib.zkfhe_last_error(None).decode() == "bfv_cts_%s: a NULL argument or a zero count" % name
    h = lib.zkfhe_bfv_evk_wide_max
    c = ctypes.c_size_t(7)
    assert h(None, ctypes.byref(prm), 8, ctypes.byref(c)) != 0 and c.value == 7
    assert lib.zkfhe_last_error(None).decode() == "bfv_evk_wide_max: a NULL argument or a zero count"


def test_python_object_needs_a_context():
    assert isinstance(zk.BfvEvalKeys, type)
    for method in ("info", "close", "__enter__", "__exit__"):
        assert callable(getattr(zk.BfvEvalKeys, method)), method
    for method in ("mul_evk", "apply_galois_evk", "slot_sum", "dot", "dot_plain"):
        assert callable(getattr(zk.BfvCiphertexts, method)), method
    assert callable(zk.Context.bfv_evk) and callable(zk.Context.bfv_evk_wide_max)
    with pytest.raises(zk.ZkfheError):
        zk.BfvEvalKeys(None)
    with pytest.raises(TypeError):
        zk.BfvEvalKeys()
