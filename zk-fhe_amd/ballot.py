"""The ballot box (zkfhe.h, bfv_ballot.hip): sums straight from the public inputs of proofs.  BallotBox, bfv_instance_words, the
helpers that lay instances out for the C ABI, and Context's bfv_sum_instances (_BallotCalls)."""
import ctypes

import numpy as np

from ._abi import BALLOT_COUNTED, BALLOT_STATUS_NAMES, BALLOT_STATUSES, ZkfheError
from .core import _Handle, call
from .hostonly import Instances, _g2_bytes


def _instance_bytes(v):
    """the public inputs of one proof as canonical 32-byte little-endian scalars: Instances, bytes, or a sequence of ints"""
    if isinstance(v, Instances):
        return v.raw
    if isinstance(v, (bytes, bytearray, memoryview)):
        b = bytes(v)
        if len(b) % 32:
            raise ValueError("instances given as bytes are a multiple of 32 long")
        return b
    return b"".join(int(x).to_bytes(32, "little") for x in v)


def _byte_arrays(blobs):
    """-> (an array of pointers to the blobs, the blobs): keep the second alive while the first is in use"""
    u8p = ctypes.POINTER(ctypes.c_uint8)
    blobs = [bytes(b) for b in blobs]
    return (u8p * max(len(blobs), 1))(*[ctypes.cast(ctypes.c_char_p(b), u8p) for b in blobs]), blobs


def _instance_arrays(items):
    """-> (pointers, scalar counts, the buffers they point into)"""
    arr, keep = _byte_arrays([_instance_bytes(v) for v in items])
    return arr, (ctypes.c_size_t * max(len(keep), 1))(*[len(b) // 32 for b in keep]), keep


def bfv_instance_words(params, instances):
    """zkfhe_bfv_instances_unpack (host only): the public inputs of one proof (Instances, bytes or a list of ints) -> (pk0, pk1, c0, c1),
    four uint64 arrays of N residues in CircuitInput order, ready for the evaluator.  Raises ZkfheError unless the item is a
    ciphertext: 5 N + 1 scalars, every one of the first 4 N a residue below Q, the rest spelling x^N + 1."""
    raw = _instance_bytes(instances)
    out = [np.empty(int(params[0]), dtype=np.uint64) for _ in range(4)]
    st = ctypes.c_int32(-1)
    call("zkfhe_bfv_instances_unpack", params, raw, len(raw) // 32, *out, ctypes.byref(st))
    if st.value != BALLOT_COUNTED:
        raise ZkfheError("bfv_instance_words: the item is not a ciphertext")
    return tuple(out)


class _BallotCalls:
    def bfv_sum_instances(self, params, items, groups=None, n_groups=1):
        """zkfhe_bfv_sum_instances: sums straight from the public inputs of proofs, WITHOUT verification.  items: one Instances,
        bytes or list of ints each; groups: one int per item (None: all 0; negative: skip).  -> (out0, out1) of shape (n_groups, N),
        counted (n_groups,) uint64 and status (n_items,) int32 (BALLOT_*).  An item that is not a ciphertext never contributes."""
        n = int(params[0])
        arr, n_inst, keep = _instance_arrays(items)   # keep: what arr points into
        k, ng = len(keep), int(n_groups)
        grp = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        if grp is not None and grp.shape != (k,):
            raise ValueError("groups must hold one integer per item")
        rows = ng if 1 <= ng <= 4096 else 1   # else the call refuses n_groups
        out0, out1 = (np.zeros((rows, n), dtype=np.uint64) for _ in range(2))
        counted, status = np.zeros(rows, dtype=np.uint64), np.zeros(max(k, 1), dtype=np.int32)
        self._call("zkfhe_bfv_sum_instances", params, k, arr, n_inst, grp, ng, out0, out1, counted, status)
        return out0, out1, counted, status[:k]


class BallotBox(_Handle):
    """zkfhe_bfv_box: a tally resident on ctx's device.  add() takes (instances, proof) pairs and counts exactly the proofs that were
    made for this election's public key (pk0, pk1), verify under vk_bytes, carry residues below Q and do not repeat the ciphertext
    of a ballot counted before; tally() reads the sums per group.  srs_seed / g2 / s_g2 as bfv_verify_batch."""
    _noun, _destroy = "ballot box", "zkfhe_bfv_box_destroy"

    def __init__(self, ctx, vk_bytes, params, pk0, pk1, n_groups=1, srs_seed=b"zkfhe-unsafe-srs", g2=None, s_g2=None):
        if (g2 is None) != (s_g2 is None):
            raise ValueError("BallotBox: give both g2 and s_g2, or neither")
        self.ctx, self.h = ctx, None
        self.params = tuple(int(x) for x in params)
        self.n_groups = int(n_groups)
        n = self.params[0]
        pk0 = np.ascontiguousarray(pk0, dtype=np.uint64)
        pk1 = np.ascontiguousarray(pk1, dtype=np.uint64)
        if pk0.shape != (n,) or pk1.shape != (n,):
            raise ValueError("pk0 / pk1 must hold N coefficients")
        seed = bytes(srs_seed) if (srs_seed is not None and g2 is None) else None
        h = ctypes.c_void_p()
        vk_bytes = bytes(vk_bytes)
        ctx._call("zkfhe_bfv_box_create", vk_bytes, len(vk_bytes), self.params, pk0, pk1, self.n_groups, seed, len(seed) if seed else 0,
                  _g2_bytes(g2) if g2 is not None else None, _g2_bytes(s_g2) if s_g2 is not None else None, ctypes.byref(h))
        self.h = h

    def add(self, items, groups=None, ctx=None):
        """zkfhe_bfv_box_add: items = [(instances, proof), ...], groups one int per item (None: all 0) -> [(status, why), ...] with
        status one of BALLOT_* and why the verifier's reason for a BALLOT_REJECTED proof.  ctx: any context of the box's device."""
        ctx = ctx or self.ctx
        box = self._handle()
        items = list(items)
        k = len(items)
        inst, n_inst, keep_i = _instance_arrays([i for i, _ in items])
        proofs, keep_p = _byte_arrays([p for _, p in items])
        lens = (ctypes.c_size_t * max(k, 1))(*[len(b) for b in keep_p])
        grp = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        if grp is not None and grp.shape != (k,):
            raise ValueError("groups must hold one integer per item")
        status = np.zeros(max(k, 1), dtype=np.int32)
        stride = 256
        errs = ctypes.create_string_buffer(stride * max(k, 1))
        ctx._call("zkfhe_bfv_box_add", box, k, inst, n_inst, proofs, lens, grp, status, errs, stride)
        del keep_i, keep_p
        return [(int(status[j]), errs.raw[j * stride:(j + 1) * stride].split(b"\0", 1)[0].decode()) for j in range(k)]

    def tally(self, ctx=None):
        """zkfhe_bfv_box_tally -> (c0, c1) of shape (n_groups, N) and counted (n_groups,): the sums so far; the box is unchanged"""
        ctx = ctx or self.ctx
        n = self.params[0]
        c0, c1 = (np.empty((self.n_groups, n), dtype=np.uint64) for _ in range(2))
        counted = np.empty(self.n_groups, dtype=np.uint64)
        ctx._call("zkfhe_bfv_box_tally", self._handle(), c0, c1, counted)
        return c0, c1, counted

    def tally_cts(self, ctx=None, out=None):
        """zkfhe_bfv_box_tally_cts -> (cts, counted): the sums so far as a resident batch of n_groups ciphertexts (out, or a fresh
        batch), copied on the device, and counted (n_groups,); the box is unchanged"""
        ctx = ctx or self.ctx
        box = self._handle()
        dst = out if out is not None else ctx.bfv_cts_zeros(self.params, self.n_groups)
        counted = np.empty(self.n_groups, dtype=np.uint64)
        try:
            ctx._call("zkfhe_bfv_box_tally_cts", box, dst._handle(), counted)
        except Exception:
            if out is None:
                dst.close()
            raise
        return dst, counted

    @property
    def totals(self):
        """zkfhe_bfv_box_info: the number of proofs per final status over every completed add, keyed by BALLOT_STATUS_NAMES"""
        t = (ctypes.c_uint64 * BALLOT_STATUSES)()
        call("zkfhe_bfv_box_info", self._handle(), None, None, t)
        return {name: int(t[i]) for i, name in enumerate(BALLOT_STATUS_NAMES)}
