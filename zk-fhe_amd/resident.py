"""What stays on the device between calls (zkfhe.h: resident batches, resident evaluation keys, prepared plans): BfvEvalKeys,
BfvCiphertexts, BfvLinearPlan and Context's factories for them, _ResidentCalls."""
import ctypes

import numpy as np

from ._abi import BfvParamsC, ZkfheError, params_tuple
from .core import _CoreCalls, _Handle, call


class _ResidentCalls:
    # ---- prepared plans: the keys and diagonals of a linear transform checked, uploaded and transformed once

    def bfv_plan(self, params, elements, gk0, gk1, diagonals, base_bits=16):
        """zkfhe_bfv_plan_create: the arguments of bfv_linear_transform without the ciphertexts -> a BfvLinearPlan, resident on this
        context's device until it is closed; plan.apply(c0, c1) is bit for bit bfv_linear_transform with these arguments."""
        g, gk0, gk1 = self._elements(params, elements, gk0, gk1, base_bits)
        d = np.ascontiguousarray(diagonals, dtype=np.uint64)
        if d.shape != (g.shape[0], int(params[0])):
            raise ValueError("diagonals must have shape (K, N), one plaintext per element")
        h = ctypes.c_void_p()
        self._call("zkfhe_bfv_plan_create", params, g.shape[0], g, gk0, gk1, int(base_bits), d, ctypes.byref(h))
        return BfvLinearPlan(self, h)

    def bfv_plan_bsgs(self, params, baby_elements, bk0, bk1, giant_elements, hk0, hk1, diagonals, base_bits=16):
        """zkfhe_bfv_plan_create_bsgs: the arguments of bfv_linear_transform_bsgs without the ciphertexts -> a BfvLinearPlan;
        plan.apply(c0, c1) is bit for bit bfv_linear_transform_bsgs with these arguments."""
        gb, bk0, bk1 = self._elements(params, baby_elements, bk0, bk1, base_bits)
        gg, hk0, hk1 = self._elements(params, giant_elements, hk0, hk1, base_bits)
        d = np.ascontiguousarray(diagonals, dtype=np.uint64)
        if d.shape != (gg.shape[0], gb.shape[0], int(params[0])):
            raise ValueError("diagonals must have shape (n_giant, n_baby, N), one plaintext per pair of elements")
        h = ctypes.c_void_p()
        self._call("zkfhe_bfv_plan_create_bsgs", params, gb.shape[0], gb, bk0, bk1, gg.shape[0], gg, hk0, hk1, int(base_bits), d, ctypes.byref(h))
        return BfvLinearPlan(self, h)

    # ---- resident batches: ciphertexts kept on the device between calls (zkfhe.h, bfv_resident.hip)

    def bfv_cts(self, params, c0, c1):
        """zkfhe_bfv_cts_upload: n ciphertexts (n, N) -> a BfvCiphertexts on this context's device; every coefficient is checked
        below Q on the device, and a batch is never created from anything else."""
        c0, c1 = self._eval_arrays(params, c0, c1)
        h = ctypes.c_void_p()
        self._call("zkfhe_bfv_cts_upload", params, c0.shape[0], c0, c1, ctypes.byref(h))
        return BfvCiphertexts(self, h)

    def bfv_cts_zeros(self, params, n):
        """zkfhe_bfv_cts_alloc: a BfvCiphertexts of n ciphertexts of zero (a destination for the calls on batches)"""
        h = ctypes.c_void_p()
        self._call("zkfhe_bfv_cts_alloc", params, int(n), ctypes.byref(h))
        return BfvCiphertexts(self, h)

    # ---- resident evaluation keys: checked, uploaded and transformed once (zkfhe.h, bfv_evk.hip)

    def bfv_evk(self, params, base_bits=16, rlk=None, elements=(), gk0=None, gk1=None):
        """zkfhe_bfv_evk_create: rlk = (rlk0, rlk1) of shape (l, N) or None; elements: Galois elements with their keys stacked as gk0,
        gk1 of shape (len(elements), l, N) -> a BfvEvalKeys, resident on this context's device until it is closed."""
        r0 = r1 = None
        if rlk is not None:
            r0, r1 = self._galois_keys(params, rlk[0], rlk[1], base_bits, ())
        g = np.ascontiguousarray([int(x) for x in elements], dtype=np.uint64).reshape(-1)
        k0 = k1 = None
        if g.shape[0]:
            if gk0 is None or gk1 is None:
                raise ValueError("gk0 and gk1 hold one key per element")
            k0, k1 = self._galois_keys(params, gk0, gk1, base_bits, (g.shape[0],))
        h = ctypes.c_void_p()
        self._call("zkfhe_bfv_evk_create", params, int(base_bits), r0, r1, g.shape[0], g if g.shape[0] else None, k0, k1, ctypes.byref(h))
        return BfvEvalKeys(self, h)

    def bfv_evk_hybrid(self, params, p, base_bits=16, rlk=None, elements=(), gk=None):
        """zkfhe_bfv_evk_create_hybrid: a key set modulo Q P for the special modulus p.  rlk = (rlk0_q, rlk1_q, rlk0_p, rlk1_p) of
        shape (l, N) or None; gk = (gk0_q, gk1_q, gk0_p, gk1_p), the keys of `elements` stacked as (len(elements), l, N) -> a
        BfvEvalKeys whose key switches divide by p (special_modulus)."""
        r = [None] * 4
        if rlk is not None:
            r = list(self._galois_keys(params, rlk[0], rlk[1], base_bits, ()) + self._galois_keys(params, rlk[2], rlk[3], base_bits, ()))
        g = np.ascontiguousarray([int(x) for x in elements], dtype=np.uint64).reshape(-1)
        k = [None] * 4
        if g.shape[0]:
            if gk is None or len(gk) != 4:
                raise ValueError("gk holds the q-planes and the p-planes of one key per element")
            lead = (g.shape[0],)
            k = list(self._galois_keys(params, gk[0], gk[1], base_bits, lead) + self._galois_keys(params, gk[2], gk[3], base_bits, lead))
        h = ctypes.c_void_p()
        self._call("zkfhe_bfv_evk_create_hybrid", params, int(p), int(base_bits), *r, g.shape[0], g if g.shape[0] else None, *k, ctypes.byref(h))
        return BfvEvalKeys(self, h)

    def bfv_evk_wide_max(self, params, base_bits=16):
        """zkfhe_bfv_evk_wide_max: the largest count of ciphertexts in a chunk whose key switch takes the digit-parallel kernels on
        this device in the calls that take a BfvEvalKeys (0: never)"""
        out = ctypes.c_size_t()
        self._call("zkfhe_bfv_evk_wide_max", params, int(base_bits), ctypes.byref(out))
        return out.value


class BfvEvalKeys(_Handle):
    """A resident evaluation key set (zkfhe_bfv_evk): one relinearization key and any number of Galois keys, transformed once and
    read-only on the device.  Any Context of the same device may use it in BfvCiphertexts.mul_evk, apply_galois_evk, slot_sum and dot;
    close() (or leaving the with block) frees it, and no context may still be using it then."""
    _noun, _destroy = "key set", "zkfhe_bfv_evk_destroy"

    def __init__(self, ctx, handle=None):
        if not isinstance(ctx, _CoreCalls):
            raise ZkfheError("BfvEvalKeys needs a Context: use Context.bfv_evk")
        if not handle:
            raise ZkfheError("BfvEvalKeys wraps a key set made by Context.bfv_evk")
        self.ctx = ctx
        self.h = handle
        self.params = self.info()["params"]

    @property
    def special_modulus(self):
        """zkfhe_bfv_evk_special_modulus: the special modulus P of a hybrid set (Context.bfv_evk_hybrid), 1 for an ordinary one"""
        p = ctypes.c_uint64()
        call("zkfhe_bfv_evk_special_modulus", self._handle(), ctypes.byref(p))
        return p.value

    def info(self):
        """zkfhe_bfv_evk_info -> params (N, Q, T, B), base_bits, has_relin, elements (the Galois elements in the order of their keys)
        and device_bytes ((has_relin + len(elements)) 2 l 5 N 4)"""
        prm, w, relin, ng, nbytes = BfvParamsC(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_uint64()
        call("zkfhe_bfv_evk_info", self._handle(), ctypes.byref(prm), ctypes.byref(w), ctypes.byref(relin), ctypes.byref(ng), None,
             ctypes.byref(nbytes))
        g = np.empty(ng.value, dtype=np.uint64)
        if ng.value:
            call("zkfhe_bfv_evk_info", self._handle(), None, None, None, None, g, None)
        return {"params": params_tuple(prm), "base_bits": w.value, "has_relin": bool(relin.value), "elements": [int(x) for x in g],
                "device_bytes": nbytes.value}


class BfvCiphertexts(_Handle):
    """A resident batch (zkfhe_bfv_cts): n ciphertexts on the device, every word a residue below Q.  The methods are the evaluation
    calls on batches, bit for bit the host-array calls of Context; each takes out=None (a fresh batch is allocated) or a batch of the
    right count to write into, which may be self or the other operand except for select and sum, and ctx=None (the creating context)
    or any context of the same device.  close() (or leaving the with block) frees it."""
    _noun, _destroy = "batch", "zkfhe_bfv_cts_destroy"

    def __init__(self, ctx, handle=None):
        if not isinstance(ctx, _CoreCalls):
            raise ZkfheError("BfvCiphertexts needs a Context: use Context.bfv_cts or Context.bfv_cts_zeros")
        if not handle:
            raise ZkfheError("BfvCiphertexts wraps a batch made by Context.bfv_cts or Context.bfv_cts_zeros")
        self.ctx = ctx
        self.h = handle
        info = self.info()
        self.params, self.n = info["params"], info["n"]

    def __len__(self):
        return self.n

    def info(self):
        """zkfhe_bfv_cts_info -> params (N, Q, T, B), n and device_bytes (16 n N)"""
        prm, n, nbytes = BfvParamsC(), ctypes.c_size_t(), ctypes.c_uint64()
        call("zkfhe_bfv_cts_info", self._handle(), ctypes.byref(prm), ctypes.byref(n), ctypes.byref(nbytes))
        return {"params": params_tuple(prm), "n": n.value, "device_bytes": nbytes.value}

    def _out(self, out, ctx, n=None):
        """the destination of a call: out, or a fresh batch of n ciphertexts (default: as many as self)"""
        return out if out is not None else (ctx or self.ctx).bfv_cts_zeros(self.params, self.n if n is None else n)

    def _into(self, out, ctx, n, fn, *args):
        """fn(ctx, *args, dst) into out or a fresh batch, which is closed again if the call is refused"""
        dst = self._out(out, ctx, n)
        try:
            (ctx or self.ctx)._call(fn, *args, dst._handle())
        except Exception:
            if out is None:
                dst.close()
            raise
        return dst

    def download(self, first=0, count=None, ctx=None):
        """zkfhe_bfv_cts_download -> (c0, c1) of shape (count, N): ciphertexts first ... first + count - 1 (default: to the end)"""
        count = self.n - int(first) if count is None else int(count)
        out = [np.empty((max(count, 0), self.params[0]), dtype=np.uint64) for _ in range(2)]
        (ctx or self.ctx)._call("zkfhe_bfv_cts_download", self._handle(), int(first), count, *out)
        return tuple(out)

    def store(self, c0, c1, first=0, ctx=None):
        """zkfhe_bfv_cts_store: ciphertexts (count, N) over ciphertexts first ... first + count - 1, checked below Q on the device
        first; a refused store leaves the batch as it was"""
        c0, c1 = self.ctx._eval_arrays(self.params, c0, c1)
        (ctx or self.ctx)._call("zkfhe_bfv_cts_store", self._handle(), int(first), c0.shape[0], c0, c1)

    def add(self, other, out=None, ctx=None, subtract=False):
        """zkfhe_bfv_cts_add: self + other (or self - other)"""
        return self._into(out, ctx, None, "zkfhe_bfv_cts_add", self._handle(), other._handle(), int(bool(subtract)))

    def sub(self, other, out=None, ctx=None):
        """zkfhe_bfv_cts_add with subtract: self - other"""
        return self.add(other, out=out, ctx=ctx, subtract=True)

    def _plain_op(self, fn, m, out, ctx):
        m = self.ctx._plain(self.params, m, self.n)
        return self._into(out, ctx, None, fn, self._handle(), m.shape[0], m)

    def add_plain(self, m, out=None, ctx=None):
        """zkfhe_bfv_cts_add_plain; m is one plaintext (N,) for every ciphertext or one per ciphertext (n, N)"""
        return self._plain_op("zkfhe_bfv_cts_add_plain", m, out, ctx)

    def mul_plain(self, m, out=None, ctx=None):
        """zkfhe_bfv_cts_mul_plain; m as for add_plain"""
        return self._plain_op("zkfhe_bfv_cts_mul_plain", m, out, ctx)

    def mul(self, other, rlk0, rlk1, base_bits=16, out=None, ctx=None):
        """zkfhe_bfv_cts_mul: the relinearized products self * other under the key (rlk0, rlk1) of shape (l, N)"""
        rlk0, rlk1 = self.ctx._galois_keys(self.params, rlk0, rlk1, base_bits, ())
        return self._into(out, ctx, None, "zkfhe_bfv_cts_mul", self._handle(), other._handle(), rlk0, rlk1, int(base_bits))

    def apply_galois(self, g, gk0, gk1, base_bits=16, out=None, ctx=None):
        """zkfhe_bfv_cts_apply_galois: sigma_g of every ciphertext, key-switched back with (gk0, gk1) of shape (l, N)"""
        gk0, gk1 = self.ctx._galois_keys(self.params, gk0, gk1, base_bits, ())
        return self._into(out, ctx, None, "zkfhe_bfv_cts_apply_galois", self._handle(), int(g), gk0, gk1, int(base_bits))

    def select(self, indices, out=None, ctx=None):
        """zkfhe_bfv_cts_select: out[j] = self[indices[j]] (repeats allowed): slice, reorder, broadcast.  out must not be self."""
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64).reshape(-1)
        return self._into(out, ctx, idx.shape[0], "zkfhe_bfv_cts_select", self._handle(), idx.shape[0], idx)

    def sum(self, groups=None, n_groups=1, out=None, ctx=None):
        """zkfhe_bfv_cts_sum: out[g] = the sum of the ciphertexts with groups[j] == g (None: all to group 0; negative: skipped); a
        batch of n_groups ciphertexts.  out must not be self."""
        grp = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        if grp is not None and grp.shape != (self.n,):
            raise ValueError("groups must hold one integer per ciphertext")
        ng = int(n_groups)
        return self._into(out, ctx, ng if 1 <= ng <= 4096 else 1, "zkfhe_bfv_cts_sum", self._handle(), grp, ng)

    # ---- the calls that take a resident key set (BfvEvalKeys): no key is checked, uploaded or transformed per call

    def mul_evk(self, other, evk, out=None, ctx=None):
        """zkfhe_bfv_cts_mul_evk: the relinearized products self * other under the set's relinearization key; bit for bit mul"""
        return self._into(out, ctx, None, "zkfhe_bfv_cts_mul_evk", self._handle(), other._handle(), evk._handle())

    def apply_galois_evk(self, g, evk, out=None, ctx=None):
        """zkfhe_bfv_cts_apply_galois_evk: sigma_g of every ciphertext with the set's key for g; bit for bit apply_galois"""
        return self._into(out, ctx, None, "zkfhe_bfv_cts_apply_galois_evk", self._handle(), int(g), evk._handle())

    def slot_sum(self, evk, out=None, ctx=None):
        """zkfhe_bfv_cts_slot_sum: every slot of every ciphertext holds its total, with the set's keys for bfv_slot_sum_elements; bit
        for bit Context.bfv_slot_sum, as one call"""
        return self._into(out, ctx, None, "zkfhe_bfv_cts_slot_sum", self._handle(), evk._handle())

    def _groups(self, n_terms):
        n_terms = int(n_terms)
        return n_terms, (self.n // n_terms if n_terms > 0 and self.n % n_terms == 0 else 1)

    def dot(self, other, n_terms, evk, out=None, ctx=None):
        """zkfhe_bfv_cts_dot: self holds n_groups * n_terms ciphertexts in [group][term] order, other n_terms (shared by every group)
        or as many as self -> n_groups inner products, one rescale and one relinearization each; out must not be a source"""
        n_terms, n_groups = self._groups(n_terms)
        return self._into(out, ctx, n_groups, "zkfhe_bfv_cts_dot", self._handle(), other._handle(), n_terms, evk._handle())

    def dot_plain(self, m, n_terms, out=None, ctx=None):
        """zkfhe_bfv_cts_dot_plain: self as for dot; m: plaintexts (n_terms, N), shared by every group, or (n_groups, n_terms, N) ->
        n_groups weighted sums; out must not be self"""
        n_terms, n_groups = self._groups(n_terms)
        m = np.ascontiguousarray(m, dtype=np.uint64)
        if m.ndim not in (2, 3) or m.shape[-1] != self.params[0] or m.shape[-2] != n_terms or 0 in m.shape:
            raise ValueError("m must have shape (n_terms, N) or (n_groups, n_terms, N)")
        return self._into(out, ctx, n_groups, "zkfhe_bfv_cts_dot_plain", self._handle(), n_terms, 1 if m.ndim == 2 else m.shape[0], m)

    # ---- ring packing (zkfhe.h "Ring packing")

    def mul_monomial(self, k, out=None, ctx=None):
        """zkfhe_bfv_cts_mul_monomial: x^k times every ciphertext; k one exponent below 2N or one per ciphertext; out may be self"""
        k = self.ctx._exponents(k, "k")
        return self._into(out, ctx, None, "zkfhe_bfv_cts_mul_monomial", self._handle(), k.shape[0], k)

    def pack(self, n, evk, pos=None, out=None, ctx=None):
        """zkfhe_bfv_cts_pack: self holds n_groups * n ciphertexts in [group][input] order -> n_groups ciphertexts, each the pack of
        its group's n inputs at pos (n_groups * n positions; None: all 0) with the set's keys for bfv_pack_elements; out must not
        be self"""
        n = int(n)
        n_groups = out.n if out is not None else (self.n // n if n > 0 and self.n % n == 0 else 1)
        p = None
        if pos is not None:
            p = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
            if p.size != n_groups * n:
                raise ValueError("pos must hold one position per input")
        return self._into(out, ctx, n_groups, "zkfhe_bfv_cts_pack", self._handle(), n, p, evk._handle())


class BfvLinearPlan(_Handle):
    """A prepared linear transform (zkfhe_bfv_plan): the element table, the transformed Galois keys and the transformed diagonals
    of Context.bfv_plan / Context.bfv_plan_bsgs, resident on the device and read-only.  Any Context of the same device may apply it;
    close() (or leaving the with block) frees it, and no context may still be applying it then."""
    _noun, _destroy = "plan", "zkfhe_bfv_plan_destroy"

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle
        self.params = self.info()["params"]

    def apply(self, c0, c1, ctx=None):
        """zkfhe_bfv_plan_apply: n ciphertexts (n, N) -> (out0, out1) of shape (n, N), on ctx (default: the creating context)."""
        ctx = ctx or self.ctx
        plan = self._handle()
        c0, c1 = ctx._eval_arrays(self.params, c0, c1)
        out = [np.empty(c0.shape, dtype=np.uint64) for _ in range(2)]
        ctx._call("zkfhe_bfv_plan_apply", plan, c0.shape[0], c0, c1, *out)
        return tuple(out)

    def apply_cts(self, ctx, cts, out=None):
        """zkfhe_bfv_cts_plan_apply: a resident batch through the plan, on ctx (None: the creating context) -> a BfvCiphertexts
        (out, which may be cts, or a fresh batch); bit for bit apply() on the downloaded batch"""
        ctx = ctx or self.ctx
        return cts._into(out, ctx, None, "zkfhe_bfv_cts_plan_apply", self._handle(), cts._handle())

    def info(self):
        """zkfhe_bfv_plan_info -> params (N, Q, T, B), base_bits, n_elems (n_baby of a two-level plan), n_giant (0: a flat plan),
        key_slots (the elements with g != 1) and device_bytes."""
        prm, w, counts, nbytes = BfvParamsC(), ctypes.c_int(), (ctypes.c_size_t * 3)(), ctypes.c_uint64()
        call("zkfhe_bfv_plan_info", self._handle(), ctypes.byref(prm), ctypes.byref(w), counts, ctypes.byref(nbytes))
        return {"params": params_tuple(prm), "base_bits": w.value, "n_elems": counts[0], "n_giant": counts[1], "key_slots": counts[2],
                "device_bytes": nbytes.value}
