"""The GPU prover's objects (zkfhe.h: communicators, SRS, keygen, prove, the batch verifier): Comm, Srs, BfvProvingKey and
bfv_verify_batch."""
import ctypes
import os

import numpy as np

from ._abi import ALLGATHER_FN, _U64P, ZkfheError, _BfvWordsC, load_library
from .hostonly import Instances, _g2_bytes, _g2_tuple, seed32


class Comm:
    """zkfhe_comm: the ranks that shard the commitments of one proof (one process per GPU).
    unique_id (128 bytes from Comm.unique_id() on rank 0, shared out of band): RCCL over xGMI, ncclAllGather on the context's
    stream.  all_gather (callable: bytes -> list of `world` byte strings, e.g. zk_fhe_amd.batch.all_gather_bytes over gloo):
    a host transport instead, for tests and for hosts with their own."""

    def __init__(self, ctx, rank, world, unique_id=None, all_gather=None):
        self.ctx, self.rank, self.world = ctx, rank, world
        self.h = ctypes.c_void_p()
        if world > 1 and unique_id is None and all_gather is None:
            raise ValueError("Comm(world > 1) needs a transport: unique_id= (RCCL) or all_gather= (a host all-gather callable)")
        if unique_id is None:     # host transport (or, with world == 1 and no callback, no transport at all)
            def cb(_user, send, nbytes, recv):
                try:
                    parts = all_gather(ctypes.string_at(send, nbytes))
                    data = b"".join(parts)
                    if len(data) != nbytes * world:
                        return 1
                    ctypes.memmove(recv, data, len(data))
                    return 0
                except Exception:  # noqa: BLE001  (must not propagate into C)
                    return 1
            self._cb = ALLGATHER_FN(cb)   # kept alive for the lifetime of the communicator
            ctx._call("zkfhe_comm_create_with_transport", rank, world, self._cb, None, ctypes.byref(self.h))
        else:
            ctx._call("zkfhe_comm_create", rank, world, bytes(unique_id), ctypes.byref(self.h))

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        rc = load_library().zkfhe_comm_unique_id(buf)
        if rc != 0:
            raise ZkfheError("zkfhe_comm_unique_id failed (%d): is librccl.so available?" % rc)
        return buf.raw

    def all_gather(self, send, recv, nbytes):
        """zkfhe_comm_all_gather on the context's stream: DeviceBuffer send (nbytes) -> DeviceBuffer recv (world * nbytes)"""
        self.ctx._call("zkfhe_comm_all_gather", self.h, send, recv, nbytes)

    def all_gather_async(self, send, recv, nbytes, byte_offset_send=0, byte_offset_recv=0):
        """zkfhe_comm_all_gather_async: the same collective on the communicator's own stream (behind what is queued on the context's
        stream); join() orders the context's stream or the caller behind it."""
        self.ctx._call("zkfhe_comm_all_gather_async", self.h, send.at(byte_offset_send), recv.at(byte_offset_recv), nbytes)

    def join(self, block_host=False):
        """zkfhe_comm_join: the context's stream (or, with block_host, the calling thread) waits for the collectives queued so far"""
        self.ctx._call("zkfhe_comm_join", self.h, 1 if block_host else 0)

    def point_range(self, n):
        lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
        self.ctx.lib.zkfhe_comm_point_range(self.h, n, ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    def destroy(self):
        if self.h:
            self.ctx.lib.zkfhe_comm_destroy(self.ctx.h, self.h)
            self.h = ctypes.c_void_p()


# zkfhe.h ZKFHE_SRS_HALO2_UNSAFE: as a seed it selects the reference's own derivation (ChaCha20Rng::from_seed([0; 32]))
SRS_HALO2_UNSAFE = b"halo2:ParamsKZG::setup(k, ChaCha20Rng::from_seed([0u8; 32]))"


class Srs:
    def __init__(self, ctx, k, seed=b"zkfhe-unsafe-srs", comm=None):
        """comm: a Comm -> only this rank's point range of both halves is built and every commitment of keygen / prove is
        sharded over the communicator (zkfhe_srs_create_sharded)."""
        self.ctx, self.k, self.comm = ctx, k, comm
        h = ctypes.c_void_p()
        if comm is None:
            ctx._call("zkfhe_srs_create", k, bytes(seed), len(seed), ctypes.byref(h))
        else:
            ctx._call("zkfhe_srs_create_sharded", comm.h, k, bytes(seed), len(seed), ctypes.byref(h))
        self.h = h

    @classmethod
    def from_points(cls, ctx, k, g, g_lagrange):
        """zkfhe_srs_from_points: an SRS computed elsewhere.  g, g_lagrange: (2^k, 8) uint64 arrays, affine Montgomery limbs."""
        a = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        b = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
        if a.shape[0] != 1 << k or b.shape[0] != 1 << k:
            raise ValueError("an SRS for k = %d needs 2^k points in both bases" % k)
        self = cls.__new__(cls)
        self.ctx, self.k = ctx, k
        h = ctypes.c_void_p()
        ctx._call("zkfhe_srs_from_points", k, a, b, ctypes.byref(h))
        self.h = h
        return self

    @classmethod
    def load(cls, ctx, path):
        """zkfhe_srs_load: a params/kzg_bn254_<k>.srs file (halo2 ParamsKZG RawBytes layout)"""
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        ctx._call("zkfhe_srs_load", os.fsencode(path), ctypes.byref(h))
        self.ctx, self.h, self.comm = ctx, h, None
        self.k = int.from_bytes(open(path, "rb").read(4), "little")
        return self

    @classmethod
    def from_monomial(cls, ctx, k, g, g2=None, s_g2=None):
        """zkfhe_srs_from_monomial: an SRS from a ceremony's powers g[i] = s^i G alone ((n_g, 8) uint64, n_g >= 2^k: a longer list is
        cut, halo2's downsize); g_lagrange is computed on the GPU.  g2, s_g2: as set_g2 takes them, or neither."""
        a = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        ctx._call("zkfhe_srs_from_monomial", k, a, a.shape[0], None if g2 is None else _g2_bytes(g2), None if s_g2 is None else _g2_bytes(s_g2),
                  ctypes.byref(h))
        self.ctx, self.h, self.comm, self.k = ctx, h, None, k
        return self

    @classmethod
    def load_downsized(cls, ctx, path, k):
        """zkfhe_srs_load_downsized: the SRS of 2^k points from a params file of k_file >= k (halo2's ParamsKZG::downsize): the first
        2^k powers and the G2 half are read, g_lagrange is computed on the GPU."""
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        ctx._call("zkfhe_srs_load_downsized", os.fsencode(path), k, ctypes.byref(h))
        self.ctx, self.h, self.comm, self.k = ctx, h, None, k
        return self

    def check(self, seed=None):
        """zkfhe_srs_check: 0, or the SRS_BAD_* bits of the checks that failed.  seed: 32 bytes the SRS's maker could not predict
        (None: the OS's entropy).  Says nothing about whether anyone forgot s."""
        if seed is not None and len(bytes(seed)) != 32:
            raise ValueError("the seed of Srs.check is 32 bytes")
        failed = ctypes.c_uint32()
        self.ctx._call("zkfhe_srs_check", self.h, None if seed is None else bytes(seed), ctypes.byref(failed))
        return int(failed.value)

    def save(self, path):
        self.ctx._call("zkfhe_srs_save", self.h, os.fsencode(path))

    def drop_host_copy(self):
        """zkfhe_srs_drop_host_copy: give back the host copies kept for save() (a later save() raises)."""
        self.ctx._check(self.ctx.lib.zkfhe_srs_drop_host_copy(self.h))

    def g2(self):
        """(G2, s G2) as ((x.c0, x.c1), (y.c0, y.c1)) ints: what bfv_verify(g2=, s_g2=) takes"""
        a, b = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
        if self.ctx.lib.zkfhe_srs_g2(self.h, a, b) != 0:
            raise ZkfheError("this SRS has no G2 half")
        return _g2_tuple(a.raw), _g2_tuple(b.raw)

    def set_g2(self, g2, s_g2):
        if self.ctx.lib.zkfhe_srs_set_g2(self.h, _g2_bytes(g2), _g2_bytes(s_g2)) != 0:
            raise ZkfheError("zkfhe_srs_set_g2: a point is not on the twist")

    def table_bits(self):
        """(digit width of the Lagrange half's digit-multiple table or 0, whether calls of many columns take the table path)."""
        wide = ctypes.c_int()
        bits = self.ctx.lib.zkfhe_srs_table_bits(self.h, ctypes.byref(wide))
        return int(bits), bool(wide.value)

    def table_info(self):
        """zkfhe_srs_table_info: {"bits": (monomial half, Lagrange half), "gb": resident GB of both tables, "narrowed": whether a half
        got a narrower table than its budget allowed because the device did not have the room}."""
        bits, nbytes, narrowed = (ctypes.c_int * 2)(), ctypes.c_uint64(), ctypes.c_int()
        self.ctx._check(self.ctx.lib.zkfhe_srs_table_info(self.h, bits, ctypes.byref(nbytes), ctypes.byref(narrowed)))
        return {"bits": (int(bits[0]), int(bits[1])), "gb": nbytes.value / 2.0 ** 30, "narrowed": bool(narrowed.value)}

    def destroy(self):
        if self.h:
            self.ctx.lib.zkfhe_srs_destroy(self.ctx.h, self.h)
            self.h = None


class BfvProvingKey:
    """zkfhe_bfv_keygen: fixed + sigma polynomials, commitments and extended-domain tables resident in HBM."""

    @classmethod
    def load(cls, ctx, srs, path, n_poly):
        """zkfhe_bfv_pk_load: a key written by save() (or by `bfv ... keygen`).  n_poly = N of the BFV parameters (sizes the
        instance buffer of prove())."""
        self = cls.__new__(cls)
        h = ctypes.c_void_p()
        ctx._call("zkfhe_bfv_pk_load", srs.h, os.fsencode(path), ctypes.byref(h))
        self.ctx, self.srs, self.params, self.config, self.h = ctx, srs, (int(n_poly), 0, 0, 0), None, h
        return self

    def save(self, path):
        self.ctx._call("zkfhe_bfv_pk_save", self.h, os.fsencode(path))

    def __init__(self, ctx, srs, input_json_text, params, config, replay=False):
        self.ctx, self.srs, self.params, self.config = ctx, srs, params, config
        cfg = config.to_c(replay)
        h = ctypes.c_void_p()
        ctx._call("zkfhe_bfv_keygen", srs.h, input_json_text.encode(), tuple(params), ctypes.byref(cfg), ctypes.byref(h))
        self.h = h

    def info(self):
        lib = self.ctx.lib
        d = ctypes.create_string_buffer(32)
        nf, ns = ctypes.c_uint32(), ctypes.c_uint32()
        lib.zkfhe_bfv_pk_info(self.h, d, ctypes.byref(nf), ctypes.byref(ns))
        fx = ctypes.create_string_buffer(64 * nf.value)
        sg = ctypes.create_string_buffer(64 * ns.value)
        lib.zkfhe_bfv_pk_commitments(self.h, fx, sg)

        def pts(buf, cnt):
            out = []
            for i in range(cnt):
                x = int.from_bytes(buf.raw[64 * i:64 * i + 32], "little")
                y = int.from_bytes(buf.raw[64 * i + 32:64 * i + 64], "little")
                out.append(None if (x == 0 and y == 0) else (x, y))
            return out
        bps = {}
        for i, name in enumerate(("gate0", "gate1", "rlc")):
            cnt = ctypes.c_uint32(0)
            lib.zkfhe_bfv_pk_break_points(self.h, i, None, ctypes.byref(cnt))
            arr = (ctypes.c_uint32 * max(1, cnt.value))()
            lib.zkfhe_bfv_pk_break_points(self.h, i, arr, ctypes.byref(cnt))
            bps[name] = list(arr)[: cnt.value]
        return {"vk_digest": int.from_bytes(d.raw, "little"), "fixed_commit": pts(fx, nf.value), "sigma_commit": pts(sg, ns.value),
                "break_points": bps}

    def prove(self, input_json_text, seed=None, ctx=None):
        """One proof. `ctx`: the context (stream + workspace) to run on -- several contexts of the same GPU may
        prove concurrently against this key from different threads (ctypes releases the GIL).
        seed: the 32-byte blinding seed.  Zero knowledge rests on it being fresh and secret: None draws os.urandom(32);
        a fixed seed is for reproducible tests.  Shorter seeds are zero-padded, longer ones hashed (seed32())."""
        ctx = ctx or self.ctx
        seed = os.urandom(32) if seed is None else seed32(seed)
        cap = 1 << 18
        buf = ctypes.create_string_buffer(cap)
        plen = ctypes.c_size_t()
        ninst = ctypes.c_size_t(5 * int(self.params[0]) + 8)   # 4 polynomials of N coefficients + cyclo (N + 1) are public
        tm = (ctypes.c_float * 5)()
        text = input_json_text if isinstance(input_json_text, bytes) else input_json_text.encode()
        for _ in range(2):
            ibuf = ctypes.create_string_buffer(32 * ninst.value)
            have = ninst.value
            rc = ctx.lib.zkfhe_bfv_prove(ctx.h, self.srs.h, self.h, text, seed, buf, cap, ctypes.byref(plen), ibuf, ctypes.byref(ninst), tm)
            if rc == 0 or ninst.value <= have:
                break      # otherwise: the library reported the instance count it needs -- retry once with that capacity
        ctx._check(rc)
        return buf.raw[: plen.value], Instances(ibuf.raw[: 32 * ninst.value]), list(tm)

    WORD_FIELDS = ("pk0", "pk1", "m", "u", "e0", "e1", "c0", "c1")

    def prove_words(self, words, seed=None, ctx=None):
        """zkfhe_bfv_prove_words: the input as machine words, `words` = a mapping of pk0, pk1, m, u, e0, e1, c0, c1 to N residues
        each (CircuitInput order; cyclo is x^N + 1).  Same bytes as prove() on the JSON that spells the same numbers."""
        ctx = ctx or self.ctx
        n = int(self.params[0])
        seed = os.urandom(32) if seed is None else seed32(seed)
        arrs = []
        for k in self.WORD_FIELDS:
            a = np.ascontiguousarray(words[k], dtype=np.uint64).reshape(-1)
            if a.size != n:
                raise ValueError("%s must hold N = %d words" % (k, n))
            arrs.append(a)
        w = _BfvWordsC(*[a.ctypes.data_as(_U64P) for a in arrs])
        cap = 1 << 18
        buf = ctypes.create_string_buffer(cap)
        plen = ctypes.c_size_t()
        ninst = ctypes.c_size_t(5 * n + 8)
        tm = (ctypes.c_float * 5)()
        ibuf = ctypes.create_string_buffer(32 * ninst.value)
        ctx._call("zkfhe_bfv_prove_words", self.srs.h, self.h, ctypes.byref(w), seed, buf, cap, ctypes.byref(plen), ibuf, ctypes.byref(ninst), tm)
        return buf.raw[: plen.value], Instances(ibuf.raw[: 32 * ninst.value]), list(tm)

    def encrypt_and_prove(self, pk0, pk1, m, enc_seed=None, seed=None, first_index=0, ctx=None):
        """Encrypt m (shape (N,) or (n_msgs, N), residues mod Q) under (pk0, pk1) on the GPU and prove each encryption.  Returns
        (c0, c1, proofs, instances): for one message c0, c1 of shape (N,) and one proof; otherwise lists.  enc_seed (the encryption
        randomness) and seed (the blinding of the proofs): None draws os.urandom(32); both must be secret and fresh."""
        ctx = ctx or self.ctx
        single = np.asarray(m).ndim == 1
        ct = ctx.bfv_encrypt(self.params, pk0, pk1, m, seed=enc_seed, first_index=first_index)
        proofs, insts = [], []
        for j in range(ct["c0"].shape[0]):
            words = {"pk0": pk0, "pk1": pk1, "m": np.asarray(m, dtype=np.uint64).reshape(-1, int(self.params[0]))[j]}
            words.update({k: ct[k][j] for k in ("u", "e0", "e1", "c0", "c1")})
            proof, inst, _ = self.prove_words(words, seed=None if seed is None else seed32(bytes(seed32(seed)) + j.to_bytes(8, "little")), ctx=ctx)
            proofs.append(proof)
            insts.append(inst)
        if single:
            return ct["c0"][0], ct["c1"][0], proofs[0], insts[0]
        return ct["c0"], ct["c1"], proofs, insts

    def witness_stream(self, input_json_text, gamma):
        """zkfhe_bfv_witness_stream: the phase-1 gate-context cells as the GPU generates them, as an (n_cells, 4) uint64 array
        of canonical values (little-endian limbs)."""
        text = input_json_text if isinstance(input_json_text, bytes) else input_json_text.encode()
        g = int(gamma).to_bytes(32, "little")
        n = ctypes.c_size_t()
        self.ctx._call("zkfhe_bfv_witness_stream", self.h, text, g, None, 0, ctypes.byref(n))
        out = np.empty((n.value, 4), dtype=np.uint64)
        self.ctx._call("zkfhe_bfv_witness_stream", self.h, text, g, out, n.value, ctypes.byref(n))
        return out

    def prefix_cache(self, capacity=-1):
        """zkfhe_bfv_pk_prefix_cache: the per-public-key transcript cache of this key (state after vk digest | pk0 | pk1).
        capacity >= 0 sets the number of public keys remembered (0 = off); returns {"hits", "misses", "entries"}."""
        h, m, e = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._check(self.ctx.lib.zkfhe_bfv_pk_prefix_cache(self.h, int(capacity), ctypes.byref(h), ctypes.byref(m), ctypes.byref(e)))
        return {"hits": h.value, "misses": m.value, "entries": e.value}

    def prehash(self, input_json_text=None):
        """zkfhe_bfv_pk_prehash: announce the input of a LATER proof -- its public inputs are absorbed into a transcript state on a
        helper thread now (host only) and the prove() of the same text starts from it.  One-shot.  Returns {"started", "taken",
        "pending"}; None as text only reads the counters."""
        s, t, p = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        text = None if input_json_text is None else (input_json_text if isinstance(input_json_text, bytes) else input_json_text.encode())
        rc = self.ctx.lib.zkfhe_bfv_pk_prehash(self.h, text, ctypes.byref(s), ctypes.byref(t), ctypes.byref(p))
        if rc != 0:
            raise ZkfheError("zkfhe_bfv_pk_prehash: too many announced proofs are pending (%d)" % rc)
        return {"started": s.value, "taken": t.value, "pending": p.value}

    def export_vk(self):
        lib = self.ctx.lib
        n = ctypes.c_size_t()
        lib.zkfhe_bfv_pk_export_vk(self.h, None, 0, ctypes.byref(n))
        buf = ctypes.create_string_buffer(n.value)
        self.ctx._check(lib.zkfhe_bfv_pk_export_vk(self.h, buf, n.value, ctypes.byref(n)))
        return buf.raw

    def destroy(self):
        if self.h:
            self.ctx.lib.zkfhe_bfv_pk_destroy(self.ctx.h, self.h)
            self.h = None


def bfv_verify_batch(ctx, vk_bytes, items, srs_seed=b"zkfhe-unsafe-srs", g2=None, s_g2=None):
    """Batch verifier (zkfhe_bfv_verify_batch): items = [(instances, proof), ...] under one verifying key, checked on ctx's GPU with
    one pairing; returns [(accepted, reason), ...], for each proof exactly what bfv_verify answers.  g2 / s_g2 as bfv_verify."""
    lib = load_library()
    items = list(items)
    n = len(items)
    enc_inst = lambda v: v.raw if isinstance(v, Instances) else b"".join(int(x).to_bytes(32, "little") for x in v)  # noqa: E731
    insts = [enc_inst(i) for i, _ in items]
    proofs = [bytes(p) for _, p in items]
    keep = insts + proofs   # the buffers below point into these
    u8p = ctypes.POINTER(ctypes.c_uint8)
    as_p = lambda b: ctypes.cast(ctypes.c_char_p(b), u8p)  # noqa: E731
    inst_arr = (u8p * max(n, 1))(*[as_p(b) for b in insts])
    proof_arr = (u8p * max(n, 1))(*[as_p(b) for b in proofs])
    n_inst = (ctypes.c_size_t * max(n, 1))(*[len(b) // 32 for b in insts])
    lens = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in proofs])
    ok = (ctypes.c_int * max(n, 1))()
    stride = 256
    errs = ctypes.create_string_buffer(stride * max(n, 1))
    if (g2 is None) != (s_g2 is None):
        raise ValueError("bfv_verify_batch: give both g2 and s_g2, or neither")
    seed = bytes(srs_seed) if srs_seed is not None else None
    rc = lib.zkfhe_bfv_verify_batch(ctx.h, vk_bytes, len(vk_bytes), n, inst_arr, n_inst, proof_arr, lens, seed if g2 is None else None,
                                    len(seed) if (g2 is None and seed) else 0, _g2_bytes(g2) if g2 is not None else None,
                                    _g2_bytes(s_g2) if s_g2 is not None else None, ok, errs, stride)
    del keep
    if rc != 0:
        raise ZkfheError("zkfhe_bfv_verify_batch failed (%d): %s" % (rc, lib.zkfhe_last_error(ctx.h).decode()))
    return [(bool(ok[j]), errs.raw[j * stride:(j + 1) * stride].split(b"\0", 1)[0].decode()) for j in range(n)]
