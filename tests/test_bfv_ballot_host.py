"""Host side of the ballot box (no GPU): the declarations and exports of the new entry points, the status constants, the oracles
ref_sum_instances and ref_box restated from the definitions of zkfhe.h on plain Python integers (tests/test_gpu_bfv_ballot.py imports
them), zkfhe_bfv_instances_unpack against the oracle on the committed input and on every malformed shape, and the refusals of
zkfhe_bfv_sum_instances and zkfhe_bfv_box_create that need no device."""
import ctypes
import hashlib
import json
import os
import random
import re

import numpy as np
import pytest

import zk_fhe_amd as zk
from tests.test_bfv_eval_host import Q29, Q60, Q63

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zkfhe_bfv_instances_unpack", "zkfhe_bfv_sum_instances", "zkfhe_bfv_box_create", "zkfhe_bfv_box_add", "zkfhe_bfv_box_tally",
               "zkfhe_bfv_box_info", "zkfhe_bfv_box_destroy"]
STATUS_NAMES = ["COUNTED", "SKIPPED", "BAD_GROUP", "NOT_A_CIPHERTEXT", "WRONG_KEY", "REJECTED", "REPEATED"]
K13 = (1024, Q29, 7, 19)


# ---- the oracles -------------------------------------------------------------------------------------------------------------

def make_instances(params, pk0, pk1, c0, c1):
    """pk0 | pk1 | c0 | c1 | x^N + 1 as a list of 5 N + 1 Python integers (every polynomial in CircuitInput order)"""
    n = params[0]
    out = [int(x) for v in (pk0, pk1, c0, c1) for x in v]
    assert len(out) == 4 * n
    return out + [1] + [0] * (n - 1) + [1]


def is_ciphertext(params, inst, first_poly=2):
    """the three conditions of zkfhe.h; the residue condition on the polynomials first_poly ... 3 (2: c0 | c1; 0: all four)"""
    n, q = params[0], params[1]
    return (len(inst) == 5 * n + 1 and all(0 <= int(v) < q for v in inst[first_poly * n:4 * n])
            and [int(v) for v in inst[4 * n:]] == [1] + [0] * (n - 1) + [1])


def ref_sum_instances(params, items, groups=None, n_groups=1):
    """zkfhe_bfv_sum_instances from its definition: items as lists of integers -> (out0, out1, counted, status)"""
    n, q = params[0], params[1]
    out0 = [[0] * n for _ in range(n_groups)]
    out1 = [[0] * n for _ in range(n_groups)]
    counted, status = [0] * n_groups, []
    for j, inst in enumerate(items):
        g = 0 if groups is None else int(groups[j])
        if g < 0:
            status.append(zk.BALLOT_SKIPPED)
        elif g >= n_groups:
            status.append(zk.BALLOT_BAD_GROUP)
        elif not is_ciphertext(params, inst):
            status.append(zk.BALLOT_NOT_A_CIPHERTEXT)
        else:
            status.append(zk.BALLOT_COUNTED)
            out0[g] = [(a + int(b)) % q for a, b in zip(out0[g], inst[2 * n:3 * n])]
            out1[g] = [(a + int(b)) % q for a, b in zip(out1[g], inst[3 * n:4 * n])]
            counted[g] += 1
    return np.array(out0, dtype=np.uint64), np.array(out1, dtype=np.uint64), np.array(counted, dtype=np.uint64), np.array(status, dtype=np.int32)


def ref_box(params, pk0, pk1, n_groups, verify):
    """The ballot box from the decision order of zkfhe.h.  verify(instances, proof) -> (accepted, reason) is the proof check (the GPU
    tests pass the single host verifier).  Returns an object with add(items, groups) -> [(status, why)], tally() and totals."""
    n, q = params[0], params[1]
    key = [int(x) for x in pk0] + [int(x) for x in pk1]

    class Box:
        def __init__(self):
            self.c0 = [[0] * n for _ in range(n_groups)]
            self.c1 = [[0] * n for _ in range(n_groups)]
            self.counted = [0] * n_groups
            self.seen = set()
            self.totals = dict.fromkeys(zk.BALLOT_STATUS_NAMES, 0)

        def add(self, items, groups=None):
            out = []
            for j, (inst, proof) in enumerate(items):
                inst = [int(v) for v in inst]
                g = 0 if groups is None else int(groups[j])
                st, why = None, ""
                if not 0 <= g < n_groups:
                    st = zk.BALLOT_BAD_GROUP
                elif len(inst) != 5 * n + 1 or inst[4 * n:] != [1] + [0] * (n - 1) + [1]:
                    st = zk.BALLOT_NOT_A_CIPHERTEXT
                elif inst[:2 * n] != key:
                    st = zk.BALLOT_WRONG_KEY
                else:
                    ok, why = verify(inst, proof)
                    words = inst[2 * n:4 * n]
                    if not ok:
                        st = zk.BALLOT_REJECTED
                    elif not all(v < q for v in words):
                        st = zk.BALLOT_NOT_A_CIPHERTEXT
                    else:
                        digest = hashlib.blake2b(b"".join(v.to_bytes(8, "little") for v in words), digest_size=32).digest()
                        if digest in self.seen:
                            st = zk.BALLOT_REPEATED
                        else:
                            self.seen.add(digest)
                            st = zk.BALLOT_COUNTED
                            self.c0[g] = [(a + b) % q for a, b in zip(self.c0[g], words[:n])]
                            self.c1[g] = [(a + b) % q for a, b in zip(self.c1[g], words[n:])]
                            self.counted[g] += 1
                self.totals[zk.BALLOT_STATUS_NAMES[st]] += 1
                out.append((st, why if st == zk.BALLOT_REJECTED else ""))
            return out

        def tally(self):
            return np.array(self.c0, dtype=np.uint64), np.array(self.c1, dtype=np.uint64), np.array(self.counted, dtype=np.uint64)

    return Box()


def malformed(params, good):
    """one item per way of not being a ciphertext, made from the good item `good` (a list of integers)"""
    n, q = params[0], params[1]

    def poke(pos, value):
        v = list(good)
        v[pos] = value
        return v
    return {
        "5N instances": good[:-1],
        "5N + 2 instances": good + [0],
        "a scalar equal to Q": poke(2 * n + 3, q),
        "limb 1 = 1 over a small limb 0": poke(3 * n + 1, (1 << 64) + 5),
        "limb 3 set": poke(4 * n - 1, (1 << 192) + 5),
        "the leading 1 of the tail missing": poke(4 * n, 0),
        "constant term 2": poke(5 * n, 2),
    }


def random_item(rng, params, pk=None):
    n, q = params[0], params[1]
    pick = lambda: [rng.randrange(q) for _ in range(n)]  # noqa: E731
    pk0, pk1 = pk if pk is not None else (pick(), pick())
    return make_instances(params, pk0, pk1, pick(), pick())


# ---- tests -------------------------------------------------------------------------------------------------------------------

def header():
    return open(os.path.join(ROOT, "include", "zkfhe.h")).read()


def test_new_symbols_declared_and_exported():
    h = header()
    lib = zk.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, h), s
        assert s in zk.EXPORTS, s
        assert hasattr(lib, s), s
    assert re.search(r"#define ZKFHE_PROF_BFV_BALLOT 24\b", h) and zk.PROF_BFV_BALLOT == 24
    assert callable(zk.Context.bfv_sum_instances) and callable(zk.bfv_instance_words)
    for name in ("add", "tally", "totals", "close"):
        assert hasattr(zk.BallotBox, name), name


def test_status_constants_equal_the_header():
    h = header()
    for value, name in enumerate(STATUS_NAMES):
        m = re.search(r"#define ZKFHE_BALLOT_%s (\d+)\b" % name, h)
        assert m and int(m.group(1)) == value == getattr(zk, "BALLOT_" + name), name
    assert zk.BALLOT_COUNTED == 0
    m = re.search(r"#define ZKFHE_BALLOT_STATUSES (\d+)\b", h)
    assert int(m.group(1)) == zk.BALLOT_STATUSES == len(STATUS_NAMES) == len(zk.BALLOT_STATUS_NAMES)
    assert [s.upper() for s in zk.BALLOT_STATUS_NAMES] == STATUS_NAMES


def golden_instances():
    inp = json.load(open(os.path.join(ROOT, "tests", "golden", "bfv", "bfv.in")))
    return [int(x) for k in ("pk0", "pk1", "c0", "c1", "cyclo") for x in inp[k]], inp


def test_unpack_the_committed_input():
    inst, inp = golden_instances()
    assert len(inst) == 5 * 1024 + 1 and is_ciphertext(K13, inst, 0)
    for form in (inst, zk.Instances(b"".join(v.to_bytes(32, "little") for v in inst)), b"".join(v.to_bytes(32, "little") for v in inst)):
        got = zk.bfv_instance_words(K13, form)
        for arr, k in zip(got, ("pk0", "pk1", "c0", "c1")):
            assert arr.dtype == np.uint64 and [int(x) for x in arr] == [int(x) for x in inp[k]], k


def unpack_status(params, inst, outputs=True):
    lib = zk.load_library()
    raw = b"".join(int(v).to_bytes(32, "little") for v in inst)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    out = [np.full(params[0], 77, dtype=np.uint64) for _ in range(4)]
    st = ctypes.c_int32(-1)
    rc = lib.zkfhe_bfv_instances_unpack(ctypes.byref(zk.BfvParamsC(*params)), raw, len(inst),
                                        *[a.ctypes.data_as(u64p) if outputs else None for a in out], ctypes.byref(st))
    return rc, st.value, out


@pytest.mark.parametrize("params", [(8, Q29, 7, 19), (8, Q63, 2, 1), (16, Q60, 65537, 19)])
def test_unpack_malformed_shapes(params):
    n, q = params[0], params[1]
    rng = random.Random(n + q % 1000)
    good = random_item(rng, params)
    good[2 * n] = q - 1                                     # the largest residue
    rc, st, out = unpack_status(params, good)
    assert (rc, st) == (0, zk.BALLOT_COUNTED) and is_ciphertext(params, good, 0)
    assert [int(x) for a in out for x in a] == good[:4 * n]
    assert unpack_status(params, good, outputs=False)[:2] == (0, zk.BALLOT_COUNTED)    # outputs may be NULL
    bad = malformed(params, good)
    bad["a key scalar equal to Q"] = good[:5] + [q] + good[6:]                          # all four polynomials are checked here
    bad["a key scalar above 2^64"] = good[:n + 2] + [1 << 64] + good[n + 3:]
    bad["no instances"] = []
    for name, inst in bad.items():
        assert not is_ciphertext(params, inst, 0), name
        rc, st, out = unpack_status(params, inst)
        assert (rc, st) == (0, zk.BALLOT_NOT_A_CIPHERTEXT), name
        assert all(int(x) == 77 for a in out for x in a), name                          # nothing written
        with pytest.raises(zk.ZkfheError, match="not a ciphertext"):
            zk.bfv_instance_words(params, inst)


def test_unpack_refusals():
    lib = zk.load_library()
    good = random_item(random.Random(1), (8, 97, 5, 1))
    with pytest.raises(zk.ZkfheError, match="bfv params"):
        zk.bfv_instance_words((12, 97, 5, 1), good)
    rc = lib.zkfhe_bfv_instances_unpack(None, b"", 0, None, None, None, None, None)
    assert rc == -1 and lib.zkfhe_last_error(None).decode().startswith("bfv_instances_unpack: ")
    # without a status word an item that is not a ciphertext is an error
    raw = b"".join(v.to_bytes(32, "little") for v in good[:-1])
    rc = lib.zkfhe_bfv_instances_unpack(ctypes.byref(zk.BfvParamsC(8, 97, 5, 1)), raw, len(good) - 1, None, None, None, None, None)
    assert rc == -1 and "not a ciphertext" in lib.zkfhe_last_error(None).decode()


def test_reference_sum_small_case():
    params = (8, 97, 5, 1)
    n, q = 8, 97
    rng = random.Random(3)
    items = [random_item(rng, params) for _ in range(5)]
    items[1][2 * n] = q          # not a residue
    groups = [0, 0, 2, -1, 3]
    out0, out1, counted, status = ref_sum_instances(params, items, groups, 3)
    assert list(status) == [zk.BALLOT_COUNTED, zk.BALLOT_NOT_A_CIPHERTEXT, zk.BALLOT_COUNTED, zk.BALLOT_SKIPPED, zk.BALLOT_BAD_GROUP]
    assert list(counted) == [1, 0, 1]
    assert [int(x) for x in out0[0]] == items[0][2 * n:3 * n] and [int(x) for x in out1[2]] == items[2][3 * n:4 * n]
    assert not out0[1].any() and not out1[1].any()
    two = ref_sum_instances(params, [items[0], items[2]])
    assert [int(x) for x in two[0][0]] == [(a + b) % q for a, b in zip(items[0][2 * n:3 * n], items[2][2 * n:3 * n])]


def test_reference_box_decision_order():
    params = (8, 97, 5, 1)
    n = 8
    rng = random.Random(4)
    pk = ([rng.randrange(97) for _ in range(n)], [rng.randrange(97) for _ in range(n)])
    v = random_item(rng, params, pk)
    other = random_item(rng, params, pk)
    foreign = random_item(rng, params)
    verify = lambda inst, proof: (proof == b"ok", "" if proof == b"ok" else "bad proof")  # noqa: E731
    box = ref_box(params, pk[0], pk[1], 2, verify)
    got = box.add([(v, b"forged"), (v, b"ok"), (other, b"ok"), (foreign, b"ok"), (v, b"ok"), (other, b"ok"), (v[:-1], b"ok")], [0, 0, 1, 0, 1, 2, 5])
    assert got == [(zk.BALLOT_REJECTED, "bad proof"), (zk.BALLOT_COUNTED, ""), (zk.BALLOT_COUNTED, ""), (zk.BALLOT_WRONG_KEY, ""),
                   (zk.BALLOT_REPEATED, ""), (zk.BALLOT_BAD_GROUP, ""), (zk.BALLOT_BAD_GROUP, "")]
    c0, c1, counted = box.tally()
    assert list(counted) == [1, 1] and [int(x) for x in c0[0]] == v[2 * n:3 * n] and [int(x) for x in c1[1]] == other[3 * n:4 * n]
    assert sum(box.totals.values()) == 7 and box.totals["repeated"] == 1
    assert box.add([(v[:-1], b"ok"), (v, b"ok")], None) == [(zk.BALLOT_NOT_A_CIPHERTEXT, ""), (zk.BALLOT_REPEATED, "")]


def sum_instances_rc(ctx_h, params, n_items=1, n_groups=1, null=None):
    lib = zk.load_library()
    inst = b"".join(v.to_bytes(32, "little") for v in random_item(random.Random(5), (8, 97, 5, 1)))
    u8p = ctypes.POINTER(ctypes.c_uint8)
    args = {
        "instances": (u8p * 1)(ctypes.cast(ctypes.c_char_p(inst), u8p)), "n_instances": (ctypes.c_size_t * 1)(41),
        "out0": (ctypes.c_uint64 * (8 * 4097))(), "out1": (ctypes.c_uint64 * (8 * 4097))(), "counted": (ctypes.c_uint64 * 4097)(),
        "status": (ctypes.c_int32 * 1)(),
    }
    if null:
        args[null] = None
    prm = ctypes.byref(zk.BfvParamsC(*params)) if params else None
    rc = lib.zkfhe_bfv_sum_instances(ctx_h, prm, n_items, args["instances"], args["n_instances"], None, n_groups, args["out0"], args["out1"],
                                     args["counted"], args["status"])
    return rc, lib.zkfhe_last_error(None).decode()


def test_sum_instances_refusals_without_a_device():
    good = (8, 97, 5, 1)
    for null in ("instances", "n_instances", "out0", "out1", "counted", "status"):
        rc, msg = sum_instances_rc(None, good, null=null)
        assert rc == -1 and msg == "bfv_sum_instances: a NULL argument or a zero count", null
    assert sum_instances_rc(None, None) == (-1, "bfv_sum_instances: a NULL argument or a zero count")
    assert sum_instances_rc(None, good, n_items=0) == (-1, "bfv_sum_instances: a NULL argument or a zero count")
    for n_groups in (0, 4097):
        assert sum_instances_rc(None, good, n_groups=n_groups) == (-1, "bfv_sum_instances: n_groups must be in [1, 4096]")
    for params in ((12, 97, 5, 1), (8, 1 << 63, 5, 1), (8, 97, 97, 1), (8, 97, 5, 0), (4, 97, 5, 1)):
        rc, msg = sum_instances_rc(None, params)
        assert rc == -1 and msg.startswith("bfv params: "), params
    assert sum_instances_rc(None, good) == (-1, "bfv_sum_instances: ctx is NULL")            # the last of the refusals


def box_create_rc(params, n_groups=1, null=None, seed=b"zkfhe-unsafe-srs", g2=None, s_g2=None):
    lib = zk.load_library()
    pk = (ctypes.c_uint64 * 8)()
    args = {"vk": b"ZKFHEVK2" + bytes(64), "pk0": pk, "pk1": pk, "out": ctypes.pointer(ctypes.c_void_p(1))}
    if null:
        args[null] = None
    prm = ctypes.byref(zk.BfvParamsC(*params)) if params else None
    rc = lib.zkfhe_bfv_box_create(None, args["vk"], 72 if args["vk"] else 0, prm, args["pk0"], args["pk1"], n_groups, seed, len(seed) if seed else 0,
                                  g2, s_g2, args["out"])
    if args["out"] is not None:
        assert not args["out"].contents.value            # *out is NULL after every refusal
    return rc, lib.zkfhe_last_error(None).decode()


def test_box_create_refusals_without_a_device():
    good = (8, 97, 5, 1)
    for null in ("vk", "pk0", "pk1", "out"):
        assert box_create_rc(good, null=null) == (-1, "bfv_box: a NULL argument or a zero count"), null
    assert box_create_rc(None) == (-1, "bfv_box: a NULL argument or a zero count")
    for n_groups in (0, 4097):
        assert box_create_rc(good, n_groups=n_groups) == (-1, "bfv_box: n_groups must be in [1, 4096]")
    for params in ((12, 97, 5, 1), (8, 1, 5, 1), (8, 97, 1, 1), (8, 97, 5, 1024), (1 << 16, 97, 5, 1)):
        rc, msg = box_create_rc(params)
        assert rc == -1 and msg.startswith("bfv params: "), params
    assert box_create_rc(good, g2=bytes(128)) == (-1, "bfv_box: give srs_seed, or both g2 and s_g2")
    assert box_create_rc(good) == (-1, "bfv_box: ctx is NULL")
    lib = zk.load_library()
    assert lib.zkfhe_bfv_box_info(None, None, None, None) == -1 and lib.zkfhe_last_error(None).decode() == "bfv_box: box is NULL"
    assert lib.zkfhe_bfv_box_destroy(None, None) == 0     # a NULL box is not an error
