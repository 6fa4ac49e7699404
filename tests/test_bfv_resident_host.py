"""Resident ciphertext batches without a GPU (bfv_resident.hip): the new entry points are exported and listed, the host-only calls
answer, and the Python object refuses to exist without a context."""
import ctypes
import os
import re

import pytest

import zk_fhe_amd as zk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zkfhe_bfv_cts_alloc", "zkfhe_bfv_cts_upload", "zkfhe_bfv_cts_store", "zkfhe_bfv_cts_download", "zkfhe_bfv_cts_info",
         "zkfhe_bfv_cts_destroy", "zkfhe_bfv_box_tally_cts", "zkfhe_bfv_cts_add", "zkfhe_bfv_cts_add_plain", "zkfhe_bfv_cts_mul_plain",
         "zkfhe_bfv_cts_mul", "zkfhe_bfv_cts_apply_galois", "zkfhe_bfv_cts_plan_apply", "zkfhe_bfv_cts_select", "zkfhe_bfv_cts_sum"]


def test_names_are_exported_and_declared():
    lib = zk.load_library()
    header = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    for name in NAMES:
        assert name in zk.EXPORTS, name
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"#define ZKFHE_PROF_BFV_RESIDENT 25\b", header) and zk.PROF_BFV_RESIDENT == 25


def test_info_of_null_is_refused():
    lib = zk.load_library()
    f = lib.zkfhe_bfv_cts_info
    assert f(None, None, None, None) != 0
    assert lib.zkfhe_last_error(None).decode() == "bfv_cts_info: cts is NULL"


def test_destroy_of_null_is_not_an_error():
    """as zkfhe_bfv_plan_destroy: no context and no object is nothing to do"""
    lib = zk.load_library()
    for name in ("zkfhe_bfv_plan_destroy", "zkfhe_bfv_cts_destroy"):
        f = getattr(lib, name)
        assert f(None, None) == 0, name


def test_calls_without_a_context_are_refused_before_any_device_work():
    lib = zk.load_library()
    prm = zk.BfvParamsC(8, 536870909, 7, 1)
    out = ctypes.c_void_p(1)
    f = lib.zkfhe_bfv_cts_alloc
    assert f(None, ctypes.byref(prm), 1, ctypes.byref(out)) != 0 and not out.value
    assert lib.zkfhe_last_error(None).decode() == "bfv_cts_alloc: a NULL argument or a zero count"
    g = lib.zkfhe_bfv_cts_add
    assert g(None, None, None, 0, None) != 0
    assert lib.zkfhe_last_error(None).decode() == "bfv_cts_add: a NULL argument or a zero count"


def test_python_object_needs_a_context():
    assert isinstance(zk.BfvCiphertexts, type)
    for method in ("download", "store", "info", "add", "sub", "add_plain", "mul_plain", "mul", "apply_galois", "select", "sum", "close"):
        assert callable(getattr(zk.BfvCiphertexts, method)), method
    assert callable(zk.Context.bfv_cts) and callable(zk.Context.bfv_cts_zeros)
    assert callable(zk.BfvLinearPlan.apply_cts) and callable(zk.BallotBox.tally_cts)
    with pytest.raises(zk.ZkfheError):
        zk.BfvCiphertexts(None)
    with pytest.raises(TypeError):
        zk.BfvCiphertexts()
