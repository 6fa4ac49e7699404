"""The calls that need no GPU and no Context (zkfhe.h: transcript, Poseidon, ChaCha20, the circuit's tables and mock prover, the
.snark container, the verifier), with the values they exchange: BfvConfig and Instances."""
import ctypes
import os

import numpy as np

from ._abi import BfvConfigC, BfvParamsC, ZkfheError, load_library
from .core import invoke


def version():
    return load_library().zkfhe_version().decode()


def seed32(seed):
    """The 32-byte blinding seed of zkfhe_bfv_prove from arbitrary bytes: up to 32 bytes are zero-padded, anything longer
    is hashed (BLAKE2b-256, person "zkfhe-seed") so that long seeds sharing a prefix do not collide."""
    import hashlib
    seed = bytes(seed)
    if len(seed) <= 32:
        return seed.ljust(32, b"\x00")
    return hashlib.blake2b(seed, digest_size=32, person=b"zkfhe-seed").digest()


# ----------------------------------------------------------------------------- transcript (host only)
TRANSCRIPT_ID = {"poseidon": 0, "blake2b": 1}


class HostTranscript:
    """zkfhe_transcript_*: the prover's Fiat-Shamir transcript (Poseidon as in snark-verifier, or halo2's Blake2b)."""

    def __init__(self, kind="poseidon"):
        self.lib = load_library()
        self.h = ctypes.c_void_p()
        rc = self.lib.zkfhe_transcript_create(TRANSCRIPT_ID[kind], ctypes.byref(self.h))
        if rc != 0:
            raise ZkfheError("zkfhe_transcript_create failed (%d)" % rc)

    def _call(self, name, payload):
        rc = getattr(self.lib, "zkfhe_transcript_" + name)(self.h, payload)
        if rc != 0:
            raise ZkfheError("zkfhe_transcript_%s refused its argument (%d)" % (name, rc))

    def common_scalar(self, s):
        self._call("common_scalar", int(s).to_bytes(32, "little"))

    def write_scalar(self, s):
        self._call("write_scalar", int(s).to_bytes(32, "little"))

    def common_point(self, P):
        x, y = (0, 0) if P is None else P
        self._call("common_point", x.to_bytes(32, "little") + y.to_bytes(32, "little"))

    def write_point(self, P):
        x, y = (0, 0) if P is None else P
        self._call("write_point", x.to_bytes(32, "little") + y.to_bytes(32, "little"))

    def squeeze(self):
        buf = ctypes.create_string_buffer(32)
        self._call("squeeze", buf)
        return int.from_bytes(buf.raw, "little")

    def stream(self):
        n = ctypes.c_size_t(0)
        self.lib.zkfhe_transcript_bytes(self.h, None, 0, ctypes.byref(n))
        buf = ctypes.create_string_buffer(max(1, n.value))
        self.lib.zkfhe_transcript_bytes(self.h, buf, n.value, ctypes.byref(n))
        return buf.raw[:n.value]

    def close(self):
        if self.h:
            self.lib.zkfhe_transcript_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def poseidon_permute(state):
    """one Poseidon permutation (BN254 Fr, t = 3, R_F = 8, R_P = 57) of three python ints, by the host library"""
    lib = load_library()
    buf = ctypes.create_string_buffer(b"".join(int(v).to_bytes(32, "little") for v in state), 96)
    rc = lib.zkfhe_poseidon_permute(buf)
    if rc != 0:
        raise ZkfheError("zkfhe_poseidon_permute refused its argument (%d)" % rc)
    return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(3)]


def host_hash_mode(mode=None):
    """'latency' | 'shared' | None (query): how concurrent provers' Poseidon transcripts hash (zkfhe_host_hash_mode)"""
    code = {None: -1, "latency": 0, "shared": 1}[mode]
    rc = load_library().zkfhe_host_hash_mode(code)
    if rc < 0:
        raise ZkfheError("zkfhe_host_hash_mode(%r) failed" % (mode,))
    return ["latency", "shared"][rc]


def prover_gate(n=-1):
    """zkfhe_prover_gate: proofs admitted at once to the GPU-heavy middle of a proof (0 = no gate, negative = query); returns the previous setting"""
    return int(load_library().zkfhe_prover_gate(int(n)))


def poseidon_hash_many(sequences, mode=1):
    """sponge digests of independent scalar sequences (python ints); mode 0 = single-sponge path, 1 = eight AVX-512 lanes on this
    thread, 2 = through the hash service threads (what concurrent provers use).  None when the CPU lacks AVX-512 IFMA (modes 1, 2)."""
    lib = load_library()
    flat = b"".join(int(v).to_bytes(32, "little") for s in sequences for v in s)
    counts = (ctypes.c_size_t * max(1, len(sequences)))(*[len(s) for s in sequences])
    out = ctypes.create_string_buffer(32 * max(1, len(sequences)))
    rc = lib.zkfhe_poseidon_hash_many(flat, counts, len(sequences), mode, out)
    if rc == -4:
        return None
    if rc != 0:
        raise ZkfheError("zkfhe_poseidon_hash_many failed (%d)" % rc)
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(len(sequences))]


def poseidon_constants():
    rc = ctypes.create_string_buffer(65 * 3 * 32)
    mds = ctypes.create_string_buffer(9 * 32)
    load_library().zkfhe_poseidon_constants(rc, mds)
    rcv = [int.from_bytes(rc.raw[32 * i:32 * i + 32], "little") for i in range(195)]
    mdv = [int.from_bytes(mds.raw[32 * i:32 * i + 32], "little") for i in range(9)]
    return [rcv[3 * r:3 * r + 3] for r in range(65)], [mdv[3 * i:3 * i + 3] for i in range(3)]


def chacha20_block(key, counter_nonce):
    """one ChaCha20 block (RFC 7539 2.3): key 32 bytes, counter_nonce = the four state words 12..15"""
    out = ctypes.create_string_buffer(64)
    if load_library().zkfhe_chacha20_block(bytes(key), (ctypes.c_uint32 * 4)(*counter_nonce), out) != 0:
        raise ZkfheError("zkfhe_chacha20_block refused its arguments")
    return out.raw


# ----------------------------------------------------------------------------- BFV circuit (host layer)
class BfvConfig:
    """configs/<name>.json: column counts + break points (the reference's pinning, README.md:38)."""

    def __init__(self, k, n_gate0, n_gate1, n_lookup, n_rlc, unusable_rows, lookup_bits=8, break_points=None, transcript="poseidon"):
        self.k, self.n_gate0, self.n_gate1, self.n_lookup, self.n_rlc = k, n_gate0, n_gate1, n_lookup, n_rlc
        self.unusable_rows, self.lookup_bits = unusable_rows, lookup_bits
        self.break_points = break_points  # dict gate0/gate1/rlc or None
        if transcript not in TRANSCRIPT_ID:
            raise ValueError("transcript must be 'poseidon' (the reference's) or 'blake2b'")
        self.transcript = transcript

    @staticmethod
    def from_pinning(cfg_json, transcript="poseidon"):
        p = cfg_json["params"]
        bp = cfg_json.get("break_points")
        bpd = None
        if bp:
            bpd = {"gate0": bp["gate"][0], "gate1": bp["gate"][1], "rlc": bp["rlc"]}
        return BfvConfig(p["degree"], p["num_range_advice"][0], p["num_range_advice"][1], p["num_lookup_advice"][1],
                         p["num_rlc_columns"], p["unusable_rows"], p["lookup_bits"], bpd, transcript)

    def to_c(self, replay):
        c = BfvConfigC(self.k, self.n_gate0, self.n_gate1, self.n_lookup, self.n_rlc, self.unusable_rows, self.lookup_bits)
        self._keep = []
        if self.break_points:
            for name in ("gate0", "gate1", "rlc"):
                arr = (ctypes.c_uint32 * len(self.break_points[name]))(*self.break_points[name])
                self._keep.append(arr)
                setattr(c, "bp_" + name, ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint32)))
                setattr(c, "n_bp_" + name, len(self.break_points[name]))
        c.replay = 1 if (replay and self.break_points) else 0
        c.transcript = TRANSCRIPT_ID[self.transcript]
        return c


def bfv_auto_config(input_json_text, params, k, unusable_rows=109, lookup_bits=8, transcript="poseidon"):
    """zkfhe_bfv_auto_config: the BfvConfig (column counts) the circuit needs at 2^k rows; host only."""
    lib = load_library()
    prm = BfvParamsC(*params)
    counts = (ctypes.c_uint32 * 4)()
    err = ctypes.create_string_buffer(256)
    text = input_json_text if isinstance(input_json_text, bytes) else input_json_text.encode()
    rc = lib.zkfhe_bfv_auto_config(text, ctypes.byref(prm), k, unusable_rows, lookup_bits, counts, err, 256)
    if rc != 0:
        raise ZkfheError("zkfhe_bfv_auto_config failed (%d): %s" % (rc, err.value.decode()))
    return BfvConfig(k, counts[0], counts[1], counts[2], counts[3], unusable_rows, lookup_bits, transcript=transcript)


def bfv_build_tables(input_json_text, params, config, gamma, keygen_mode, replay=False):
    """Host-only witness tables (no GPU). params = (N, Q, T, B); gamma = python int. Returns a dict of numpy arrays."""
    lib = load_library()
    prm = BfvParamsC(*params)
    cfg = config.to_c(replay)
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    rc = lib.zkfhe_bfv_build_tables(input_json_text.encode(), ctypes.byref(prm), ctypes.byref(cfg), int(gamma).to_bytes(32, "little"),
                                    int(bool(keygen_mode)), ctypes.byref(h), err, 512)
    if rc != 0:
        raise ZkfheError("zkfhe_bfv_build_tables failed (%d): %s" % (rc, err.value.decode()))
    cnt = lambda w: int(lib.zkfhe_bfv_tables_count(h, w))  # noqa: E731
    n_adv, n_fix, n, n_inst, n_cp = cnt(0), cnt(1), cnt(2), cnt(3), cnt(4)
    out = {"n": n, "cells": (cnt(8), cnt(9), cnt(10)), "lookups": cnt(11)}
    adv = np.empty((n_adv, n, 4), dtype=np.uint64)
    invoke(lib.zkfhe_bfv_tables_copy_advice, h, adv)
    out["advice"] = adv
    if n_fix:
        fx = np.empty((n_fix, n, 4), dtype=np.uint64)
        invoke(lib.zkfhe_bfv_tables_copy_fixed, h, fx)
        out["fixed"] = fx
    inst = np.empty((n_inst, 4), dtype=np.uint64)
    invoke(lib.zkfhe_bfv_tables_copy_instance, h, inst)
    out["instance"] = inst
    cp = np.empty((n_cp, 2), dtype=np.uint64)
    if n_cp:
        invoke(lib.zkfhe_bfv_tables_copy_copies, h, cp)
    out["copies"] = cp
    bps = {}
    for i, name in enumerate(("gate0", "gate1", "rlc")):
        a = np.empty(cnt(5 + i), dtype=np.uint32)
        if a.size:
            invoke(lib.zkfhe_bfv_tables_copy_break_points, h, i, a)
        bps[name] = a.tolist()
    out["break_points"] = bps
    lib.zkfhe_bfv_tables_free(h)
    return out


def bfv_mock(input_json_text, params, config, gamma=7, pokes=()):
    """`mock` (README.md:18-22): build the table (keygen mode: values, fixed columns, copy constraints) and check every
    constraint on every row.  pokes: [(advice column, row, value)] overwritten before the check (negative tests).
    Returns (number of violated rows / constraints, description of the first)."""
    lib = load_library()
    prm = BfvParamsC(*params)
    cfg = config.to_c(False)
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    g = int(gamma).to_bytes(32, "little")
    text = input_json_text if isinstance(input_json_text, bytes) else input_json_text.encode()
    rc = lib.zkfhe_bfv_build_tables(text, ctypes.byref(prm), ctypes.byref(cfg), g, 1, ctypes.byref(h), err, 512)
    if rc != 0:
        raise ZkfheError("circuit is not satisfied (%d): %s" % (rc, err.value.decode()))
    try:
        for col, row, val in pokes:
            if lib.zkfhe_bfv_tables_poke_advice(h, col, row, int(val).to_bytes(32, "little")) != 0:
                raise ZkfheError("zkfhe_bfv_tables_poke_advice refused (%d, %d)" % (col, row))
        nf = ctypes.c_uint64(0)
        rc = lib.zkfhe_bfv_mock_check(h, g, ctypes.byref(nf), err, 512)
        if rc != 0:
            raise ZkfheError("zkfhe_bfv_mock_check failed (%d): %s" % (rc, err.value.decode()))
        return int(nf.value), err.value.decode()
    finally:
        lib.zkfhe_bfv_tables_free(h)


# ----------------------------------------------------------------------------- public inputs, containers, the verifier
class Instances:
    """The public inputs of a proof: a read-only sequence of ints over the 32-byte little-endian words the C ABI returns.
    Decoded on demand -- turning 5121 words into Python ints costs more host time than the C side of a k = 13 proof
    spends outside the GPU, and holds the GIL while other proving threads wait for it."""

    __slots__ = ("raw", "_ints")

    def __init__(self, raw):
        self.raw = bytes(raw)
        self._ints = None

    def _decode(self):
        if self._ints is None:
            r = self.raw
            self._ints = [int.from_bytes(r[i:i + 32], "little") for i in range(0, len(r), 32)]
        return self._ints

    def __len__(self):
        return len(self.raw) // 32

    def __iter__(self):
        return iter(self._decode())

    def __getitem__(self, i):
        return self._decode()[i]

    def __eq__(self, other):
        if isinstance(other, Instances):
            return self.raw == other.raw
        try:
            return self._decode() == list(other)
        except TypeError:
            return NotImplemented

    def __repr__(self):
        return "Instances(%d words)" % len(self)


def _g2_tuple(b):
    v = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def _g2_bytes(p):
    """a G2 point ((x.c0, x.c1), (y.c0, y.c1)) of ints as the 128 bytes the C ABI takes"""
    return b"".join(int(v).to_bytes(32, "little") for pair in p for v in pair)


def srs_file_g2(path):
    """(k, G2, s G2) from the tail of a params/kzg_bn254_<k>.srs file; points as ((x.c0, x.c1), (y.c0, y.c1)).  Host only."""
    a, b, k = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128), ctypes.c_uint32()
    if load_library().zkfhe_srs_file_g2(os.fsencode(path), ctypes.byref(k), a, b) != 0:
        raise ZkfheError("%s is not a params file" % path)
    return k.value, _g2_tuple(a.raw), _g2_tuple(b.raw)


def snark_encode(instances, proof):
    """data/<name>.snark container (zkfhe.h zkfhe_snark_encode): instances = ints or an Instances object"""
    lib = load_library()
    inst = instances.raw if isinstance(instances, Instances) else b"".join(int(v).to_bytes(32, "little") for v in instances)
    n = len(inst) // 32
    ln = ctypes.c_size_t()
    lib.zkfhe_snark_encode(inst, n, bytes(proof), len(proof), None, 0, ctypes.byref(ln))
    out = ctypes.create_string_buffer(ln.value)
    if lib.zkfhe_snark_encode(inst, n, bytes(proof), len(proof), out, ln.value, ctypes.byref(ln)) != 0:
        raise ZkfheError("zkfhe_snark_encode: an instance is not a reduced scalar")
    return out.raw


def snark_decode(snark):
    """-> (list of instance ints, proof bytes); raises on a malformed container"""
    lib = load_library()
    n, pl = ctypes.c_size_t(), ctypes.c_size_t()
    if lib.zkfhe_snark_decode(bytes(snark), len(snark), None, ctypes.byref(n), None, ctypes.byref(pl)) != 0:
        raise ZkfheError("not a snark container")
    inst, proof = ctypes.create_string_buffer(32 * n.value + 1), ctypes.create_string_buffer(pl.value + 1)
    if lib.zkfhe_snark_decode(bytes(snark), len(snark), inst, ctypes.byref(n), proof, ctypes.byref(pl)) != 0:
        raise ZkfheError("snark container: an instance is not a reduced scalar")
    return [int.from_bytes(inst.raw[32 * i:32 * i + 32], "little") for i in range(n.value)], proof.raw[:pl.value]


def make_vk_bytes(k, n_gate0, n_gate1, n_lookup, n_rlc, unusable_rows, lookup_bits, vk_digest, fixed_commit, sigma_commit, transcript="poseidon"):
    """Serialise a verifying key (same layout as zkfhe_bfv_pk_export_vk) from python values; points are (x, y) or None."""
    import struct
    out = b"ZKFHEVK2" + struct.pack("<10I", k, n_gate0, n_gate1, n_lookup, n_rlc, unusable_rows, lookup_bits, TRANSCRIPT_ID[transcript],
                                    len(fixed_commit), len(sigma_commit))
    out += int(vk_digest).to_bytes(32, "little")
    for p in list(fixed_commit) + list(sigma_commit):
        x, y = (0, 0) if p is None else p
        out += int(x).to_bytes(32, "little") + int(y).to_bytes(32, "little")
    return out


def bfv_verify(vk_bytes, instances, proof, srs_seed=b"zkfhe-unsafe-srs", g2=None, s_g2=None):
    """Host-only verifier (C++: transcript replay, quotient identity, one pairing-product check). Returns (accepted, reason).
    g2 / s_g2: the verifier's half of an external SRS, each ((x.c0, x.c1), (y.c0, y.c1)) as ints; default: the seeded setup."""
    lib = load_library()
    inst = instances.raw if isinstance(instances, Instances) else b"".join(int(v).to_bytes(32, "little") for v in instances)
    ok = ctypes.c_int(0)
    err = ctypes.create_string_buffer(256)
    if g2 is not None or s_g2 is not None:
        rc = lib.zkfhe_bfv_verify_g2(vk_bytes, len(vk_bytes), inst, len(instances), proof, len(proof), _g2_bytes(g2), _g2_bytes(s_g2),
                                     ctypes.byref(ok), err, 256)
        if rc != 0:
            raise ZkfheError("zkfhe_bfv_verify_g2: bad arguments (%d)" % rc)
        return bool(ok.value), err.value.decode()
    rc = lib.zkfhe_bfv_verify(vk_bytes, len(vk_bytes), inst, len(instances), proof, len(proof), bytes(srs_seed), len(srs_seed), ctypes.byref(ok), err, 256)
    if rc != 0:
        raise ZkfheError("zkfhe_bfv_verify: bad arguments (%d)" % rc)
    return bool(ok.value), err.value.decode()
