"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads, and exports every symbol
that include/zkfhe.h declares, and the binding's signature table (zk-fhe_amd/_abi.py) says what the header's prototypes say
(no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

import zk_fhe_amd as zk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(zkfhe_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = zk.load_library()
    syms = declared_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(zk.EXPORTS) == syms


# ---- the signature table of zk-fhe_amd/_abi.py against the header's prototypes, parameter by parameter

ADDRESS, VOID = "address", "void"
C_CLASS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "size_t": ctypes.c_size_t}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None, "char *": ctypes.c_char_p, "void *": ctypes.c_void_p}
WORDS = {"char", "double", "float", "void", "uint8_t", "zkfhe_allgather_fn", *C_CLASS}   # with the zkfhe_* struct names: all that may be a type


def c_class(spelling, what):
    """the ABI class of one C type spelling (a parameter with its name and array suffix, or a return type)"""
    s = re.sub(r"\[[^\]]*\]", "*", spelling)   # T name[...] is T *name
    words = [w for w in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", s) if w not in ("const", "struct", "ZKFHE_API", "extern")]
    if len(words) == 2:   # a type and the parameter's name
        words = words[:1]
    assert len(words) == 1 and (words[0] in WORDS or words[0].startswith("zkfhe_")), "%s: unknown C type %r" % (what, spelling)
    if "*" in s or words[0] == "zkfhe_allgather_fn":
        return ADDRESS
    if words[0] == "void":
        return VOID
    assert words[0] in C_CLASS, "%s: unknown C type %r" % (what, spelling)
    return C_CLASS[words[0]]


def table_class(t):
    if t is None:
        return VOID
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)):
        return ADDRESS
    return t


def declared_prototypes():
    """name -> (return type, [parameters]) as the header spells them"""
    src = open(os.path.join(ROOT, "include", "zkfhe.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \*\n]*?)\b(zkfhe_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", src):
        assert name not in out, name
        params = [p.strip() for p in params.split(",")]
        out[name] = (ret, [] if params in ([""], ["void"]) else params)
    return out


def test_signature_table_follows_the_header():
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(zk.SIGNATURES)   # no entry the header lacks, no function the table lacks
    for name, (ret, params) in protos.items():
        restype, argtypes = zk.SIGNATURES[name]
        ret = " ".join(w for w in ret.replace("*", " * ").split() if w not in ("const", "ZKFHE_API", "extern"))
        assert ret in RETURNS, "%s: unknown return type %r" % (name, ret)
        assert restype is RETURNS[ret], "%s: returns %r, the table says %r" % (name, ret, restype)
        assert len(argtypes) == len(params), "%s: %d parameters, the table has %d" % (name, len(params), len(argtypes))
        for i, (p, t) in enumerate(zip(params, argtypes)):
            assert table_class(t) == c_class(p, name), "%s: parameter %d is %r, the table says %r" % (name, i, p, t)


def test_unknown_spellings_and_mismatches_are_caught():
    """the check itself: a type it does not know, a wrong width and a value where an address belongs do not pass"""
    for bad in ("long n", "unsigned x", "uint16_t v", "struct foo bar baz"):
        with pytest.raises(AssertionError):
            c_class(bad, "probe")
    assert c_class("const uint64_t *restrict_", "probe") == c_class("uint64_t out[4]", "probe") == c_class("zkfhe_ctx **out", "probe") == ADDRESS
    assert c_class("size_t n", "probe") is ctypes.c_size_t and c_class("size_t", "probe") is ctypes.c_size_t
    assert table_class(ctypes.c_int) != c_class("uint32_t k", "probe") and table_class(ctypes.c_int) != c_class("size_t n", "probe")
    assert table_class(ctypes.c_uint64) != c_class("const uint64_t *p", "probe")
    assert table_class(ctypes.POINTER(ctypes.c_uint64)) == table_class(zk.ALLGATHER_FN) == ADDRESS


def test_the_library_is_typed_by_the_table_alone():
    lib = zk.load_library()
    for name, (restype, argtypes) in zk.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype == restype and list(f.argtypes) == list(argtypes), name
    assign = re.compile(r"\.(argtypes|restype)\s*=[^=]")
    files = [os.path.join(ROOT, "__graft_entry__.py")]
    for top in ("zk-fhe_amd", "tests", "tools"):
        for base, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(base, f) for f in names if f.endswith(".py")]
    assert len(files) > 30
    bad = [os.path.relpath(f, ROOT) for f in files
           if os.path.relpath(f, ROOT) != os.path.join("zk-fhe_amd", "_abi.py") and assign.search(open(f, errors="ignore").read())]
    assert not bad, bad


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(zk.ZkfheError):
        zk.Context(0)


def test_product_does_not_reference_oracle():
    """The product tree must never import / include / link the oracle."""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "zk-fhe_amd")):
        if "_build" in base:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", ".inc")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                if re.search(r"(from|import)\s+oracle|oracle/[a-z_]+\.(h|c)\"|liboracle", txt):
                    bad.append(f)
    assert not bad, bad
