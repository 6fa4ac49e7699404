"""The context and what it owns (zkfhe.h: contexts, device memory, timers, profiling, Fr, NTT, MSM, G1 and witness calls), the one
marshaller every call goes through, and the base of the wrappers that own a library handle."""
import ctypes

import numpy as np

from ._abi import BfvParamsC, ZkfheError, load_library

_PARAMS_P = ctypes.POINTER(BfvParamsC)


class DeviceBuffer:
    """A device (HBM) allocation owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        ctx._call("zkfhe_dev_alloc", self.nbytes, ctypes.byref(p))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.ctx.lib.zkfhe_dev_free(self.ctx.h, self.ptr)
            self.ptr = None

    def at(self, byte_offset):
        return ctypes.c_void_p(self.ptr + int(byte_offset))

    def upload(self, arr, byte_offset=0):
        a = np.ascontiguousarray(arr)
        assert byte_offset + a.nbytes <= self.nbytes
        self.ctx._call("zkfhe_upload", self.at(byte_offset), a, a.nbytes)
        return self

    def download(self, dtype=np.uint64, shape=None, byte_offset=0, nbytes=None):
        nbytes = self.nbytes - byte_offset if nbytes is None else nbytes
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self.ctx._call("zkfhe_download", out, self.at(byte_offset), nbytes)
        return out.reshape(shape) if shape is not None else out

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def invoke(f, *args):
    """f(*args) with every argument converted by the parameter type that the signature table declares: a numpy array to that
    pointer type, a DeviceBuffer to its address, an (n, q, t, b) tuple to a BfvParamsC by reference; everything else (integers,
    bytes, None, byref(...), handles) is passed on as it is.  Returns what f returns."""
    conv = []
    for t, a in zip(f.argtypes, args):
        if isinstance(a, np.ndarray):
            a = a.ctypes.data_as(t)
        elif isinstance(a, DeviceBuffer):
            a = a.ptr
        elif t is _PARAMS_P and isinstance(a, (tuple, list)):
            a = ctypes.byref(BfvParamsC(*[int(x) for x in a]))
        conv.append(a)
    return f(*conv, *args[len(conv):])   # a surplus argument is ctypes' to refuse


def call(fn, *args):
    """fn(*args) for a function that takes no context; raises ZkfheError with the library's message on failure"""
    lib = load_library()
    rc = invoke(getattr(lib, fn), *args)
    if rc != 0:
        raise ZkfheError("%s failed (%d): %s" % (fn, rc, lib.zkfhe_last_error(None).decode()))


class _Handle:
    """A library object made through a context: h, None once closed; close() (or leaving the with block) calls _destroy."""
    _noun = _destroy = None

    def _handle(self):
        if not self.h:
            raise ZkfheError("the %s is closed" % self._noun)
        return self.h

    def close(self):
        if self.h:
            h, self.h = self.h, None
            self.ctx._call(self._destroy, h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Basis:
    """Device-resident MSM basis (SRS half) with its per-window tables."""

    def __init__(self, ctx, bases, window_bits=0):
        b = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        self.ctx = ctx
        h = ctypes.c_void_p()
        ctx._call("zkfhe_basis_create", b, b.shape[0], int(window_bits), ctypes.byref(h))
        self.h = h
        self.n = b.shape[0]

    @property
    def has_table(self):
        """True when the basis holds a digit-multiple table (every MSM against it is a plain sum of table points)."""
        return bool(self.ctx.lib.zkfhe_basis_has_multiples(self.h))

    def destroy(self):
        if self.h:
            self.ctx.lib.zkfhe_basis_destroy(self.ctx.h, self.h)
            self.h = None


class _CoreCalls:
    """Context's own part: creation, the status check, device memory, timers, profiling and the Fr, NTT, MSM, G1 and witness calls."""

    def __init__(self, device_id=0, stream=None):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.zkfhe_ctx_create(int(device_id), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h))
        if rc != 0:
            raise ZkfheError("zkfhe_ctx_create failed (%d): %s" % (rc, self.lib.zkfhe_last_error(None).decode()))
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise ZkfheError("zkfhe call failed (%d): %s" % (rc, self.lib.zkfhe_last_error(self.h).decode()))

    def _call(self, fn, *args):
        """fn(ctx, *args) through invoke(); raises ZkfheError with this context's message on failure"""
        self._check(invoke(getattr(self.lib, fn), self.h, *args))

    def close(self):
        if self.h:
            self.lib.zkfhe_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        self._call("zkfhe_sync")

    def device_info(self):
        name = ctypes.create_string_buffer(64)
        cu = ctypes.c_int()
        mem = ctypes.c_size_t()
        self._call("zkfhe_device_info", name, 64, ctypes.byref(cu), ctypes.byref(mem))
        return {"arch": name.value.decode(), "num_cu": cu.value, "hbm_bytes": mem.value}

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        a = np.ascontiguousarray(arr)
        return self.alloc(a.nbytes).upload(a)

    def prof_enable(self, on=True):
        self._call("zkfhe_prof_reset")
        self._call("zkfhe_prof_enable", int(bool(on)))

    def last_proof_marks(self):
        """zkfhe_ctx_last_proof_marks: ms from the start of the last proof on this context to (phase-0 commitment back from the GPU,
        first challenge squeezed, proof complete)"""
        m = (ctypes.c_float * 3)()
        self._call("zkfhe_ctx_last_proof_marks", m)
        return list(m)

    def last_proof_commands(self):
        """zkfhe_ctx_last_proof_commands: what the last proof on this context put on its streams, counted on the host"""
        c = (ctypes.c_uint64 * 3)()
        self._call("zkfhe_ctx_last_proof_commands", c)
        return {"kernel_launches": int(c[0]), "copy_commands": int(c[1]), "fill_commands": int(c[2])}

    def prof_read(self, which):
        ms, cnt, by = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_double()
        self._call("zkfhe_prof_read", which, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(by))
        ops = ctypes.c_double()
        self._call("zkfhe_prof_read_ops", which, ctypes.byref(ops))
        return {"total_ms": ms.value, "launches": cnt.value, "algorithmic_bytes": by.value, "ops": ops.value}

    def timer_start(self):
        self._call("zkfhe_timer_start")

    def timer_stop_ms(self):
        ms = ctypes.c_float()
        self._call("zkfhe_timer_stop_ms", ctypes.byref(ms))
        return ms.value

    # ---- device-resident calls (pointers are DeviceBuffer or c_void_p) ----
    @staticmethod
    def _p(x):
        return ctypes.c_void_p(x.ptr) if isinstance(x, DeviceBuffer) else x

    def fr_binop_dev(self, op, a, b, out, n):
        self._call("zkfhe_fr_" + op, a, b, out, n)

    def ntt_dev(self, cols, n_cols, log_n, inverse=False):
        self._call("zkfhe_ntt_batch", cols, n_cols, log_n, int(bool(inverse)))

    def ntt_to_dev(self, src, dst, n_cols, log_n, inverse=False):
        self._call("zkfhe_ntt_batch_to", src, dst, n_cols, log_n, int(bool(inverse)))

    def coset_ntt_dev(self, src, dst, n_cols, log_n, log_ext_factor, g, inverse=False):
        g = np.ascontiguousarray(g, dtype=np.uint64)
        self._call("zkfhe_coset_ntt_batch", src, dst, n_cols, log_n, log_ext_factor, g, int(bool(inverse)))

    def msm_dev(self, basis, scalars, n_cols, out):
        self._call("zkfhe_msm_batch", basis.h, scalars, n_cols, out)

    # ---- numpy convenience (host in, host out; used by tests and smoke) ----
    def _fr(self, a):
        return np.ascontiguousarray(a, dtype=np.uint64)

    def fr_binop(self, op, a, b):
        a, b = self._fr(a), self._fr(b)
        n = a.size // 4
        da, db = self.to_device(a), self.to_device(b)
        self.fr_binop_dev(op, da, db, da, n)
        out = da.download(shape=a.shape)
        da.free(), db.free()
        return out

    def fr_batch_invert_mul(self, num, den):
        """zkfhe_fr_batch_invert_mul: num[i] * den[i]^-1 (0 where den[i] = 0)"""
        num, den = self._fr(num), self._fr(den)
        n = num.size // 4
        dn, dd = self.to_device(num), self.to_device(den)
        self._call("zkfhe_fr_batch_invert_mul", dd, dn, n)
        out = dn.download(shape=num.shape)
        dn.free(), dd.free()
        return out

    FR9_OPS = {"mul": 0, "sqr": 1, "mul2": 2, "perm": 3, "lookup": 4, "chain": 5}

    def fr9_op(self, op, operands):
        """zkfhe_fr9_op: the nine-limb Fr arithmetic of the prover's kernels on five operand arrays (n, 4) each"""
        ops = self._fr(np.stack([self._fr(o) for o in operands]))
        assert ops.shape[0] == 5
        n = ops.shape[1]
        din, dout = self.to_device(ops), self.alloc(max(n, 1) * 32)
        self._call("zkfhe_fr9_op", self.FR9_OPS[op], din, dout, n)
        out = dout.download(shape=(n, 4))
        din.free(), dout.free()
        return out

    def fr_unop(self, name, a, *extra):
        a = self._fr(a)
        n = a.size // 4
        da = self.to_device(a)
        if name == "batch_invert":
            self._call("zkfhe_fr_batch_invert", da, n)
        elif name == "scale":
            self._call("zkfhe_fr_scale", da, self._fr(extra[0]), da, n)
        elif name == "sqr_chain":
            self._call("zkfhe_fr_sqr_chain", da, da, n, int(extra[0]))
        else:
            self._call("zkfhe_fr_" + name, da, da, n)
        out = da.download(shape=a.shape)
        da.free()
        return out

    def ntt(self, cols, log_n, inverse=False):
        a = self._fr(cols)
        n = 1 << log_n
        n_cols = a.size // 4 // n
        d = self.to_device(a)
        self.ntt_dev(d, n_cols, log_n, inverse)
        out = d.download(shape=a.shape)
        d.free()
        return out

    def coset_ntt(self, cols, log_n, log_ext_factor, g, inverse=False):
        a = self._fr(cols)
        n, ne = 1 << log_n, 1 << (log_n + log_ext_factor)
        if not inverse:
            n_cols = a.size // 4 // n
            src, dst = self.to_device(a), self.alloc(n_cols * ne * 32)
        else:
            n_cols = a.size // 4 // ne
            src, dst = self.to_device(a), self.alloc(n_cols * ne * 32)
        self.coset_ntt_dev(src, dst, n_cols, log_n, log_ext_factor, g, inverse)
        out = dst.download(shape=(n_cols, ne, 4))
        src.free(), dst.free()
        return out

    def msm(self, basis, scalars):
        s = self._fr(scalars)
        n_cols = s.size // 4 // basis.n
        ds, do = self.to_device(s), self.alloc(n_cols * 64)
        self.msm_dev(basis, ds, n_cols, do)
        out = do.download(shape=(n_cols, 8))
        ds.free(), do.free()
        return out

    def msm_xyzz(self, basis, scalars):
        """zkfhe_msm_batch_xyzz + zkfhe_g1_xyzz_to_affine: the sums in accumulator form from the GPU, ONE inversion for all of them
        on the host.  Returns (affine (n_cols, 8) uint64, raw xyzz (n_cols, 16) uint64)."""
        scalars = self._fr(scalars)
        n_cols = scalars.size // 4 // basis.n
        d = self.to_device(scalars)
        out = self.alloc(n_cols * 128)
        self._call("zkfhe_msm_batch_xyzz", basis.h, d, n_cols, out)
        raw = np.ascontiguousarray(out.download(dtype=np.uint64, shape=(n_cols, 16)))
        aff = np.empty((n_cols, 8), dtype=np.uint64)
        self._check(invoke(self.lib.zkfhe_g1_xyzz_to_affine, raw, n_cols, aff))
        d.free(), out.free()
        return aff, raw

    def msm_sharded(self, comm, basis_slice, scalars, lo):
        """zkfhe_msm_batch_sharded: `scalars` = the FULL columns (n_cols, n_full, 4); this rank's basis slice covers rows
        lo .. lo + len(basis_slice).  Every rank gets the full commitments."""
        s = self._fr(scalars)
        n_cols, n_full = s.shape[0], s.shape[1]
        ds, do = self.to_device(s), self.alloc(n_cols * 64)
        self._call("zkfhe_msm_batch_sharded", comm.h, basis_slice.h, ds.at(lo * 32), n_full, n_cols, do)
        out = do.download(shape=(n_cols, 8))
        ds.free(), do.free()
        return out

    def g1_add(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 8)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 8)
        da, db = self.to_device(a), self.to_device(b)
        self._call("zkfhe_g1_add", da, db, da, a.shape[0])
        out = da.download(shape=a.shape)
        da.free(), db.free()
        return out

    def g1_mul(self, p, k):
        p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8)
        k = np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)
        dp, dk = self.to_device(p), self.to_device(k)
        self._call("zkfhe_g1_mul", dp, dk, dp, p.shape[0])
        out = dp.download(shape=p.shape)
        dp.free(), dk.free()
        return out

    def g1_fft(self, points, inverse=False):
        """zkfhe_g1_fft: the FFT over 2^log_n G1 points ((n, 8) uint64, affine Montgomery limbs, identity = (0, 0)) with the root of
        unity of ntt(); inverse=True is halo2's g_to_lagrange (w^-1 and n^-1).  Natural order in and out."""
        p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        n = p.shape[0]
        if n < 2 or n & (n - 1):
            raise ValueError("g1_fft needs 2^log_n points, log_n >= 1")
        dp = self.to_device(p)
        try:
            self._call("zkfhe_g1_fft", dp, n.bit_length() - 1, 1 if inverse else 0)
            return dp.download(shape=p.shape)
        finally:
            dp.free()

    def g1_decompress(self, data):
        """32-byte compressed G1 points (bytes, a multiple of 32 long) -> (points (n, 8) uint64 Montgomery affine, status (n,) int32:
        0 ok, 1 x not reduced, 2 not on the curve, 3 non-canonical identity; a rejected point is (0, 0))"""
        data = bytes(data)
        if len(data) % 32:
            raise ValueError("g1_decompress: input length is not a multiple of 32")
        n = len(data) // 32
        if not n:
            return np.zeros((0, 8), dtype=np.uint64), np.zeros(0, dtype=np.int32)
        din = self.to_device(np.frombuffer(data, dtype=np.uint8))
        dout, dst = self.alloc(n * 64), self.alloc(n * 4)
        self._call("zkfhe_g1_decompress", din, n, dout, dst)
        pts, st = dout.download(shape=(n, 8)), dst.download(dtype=np.int32)
        din.free(), dout.free(), dst.free()
        return pts, st

    def msm_segmented(self, points, index, scalars, offsets):
        """out[s] = sum over t in [offsets[s], offsets[s+1]) of scalars[t] * points[index[t]]: points (n, 8) uint64 Montgomery affine,
        scalars (T, 4) uint64 Montgomery Fr, index (T,) and offsets (n_segs + 1,) integers.  Returns (n_segs, 8) affine."""
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        index = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        n_segs, T = offsets.shape[0] - 1, index.shape[0]
        if n_segs < 1 or scalars.shape[0] != T:
            raise ValueError("msm_segmented: need n_segs + 1 offsets and one scalar per index")
        bufs = [self.to_device(a) if a.size else None for a in (points, index, scalars, offsets)]
        dout = self.alloc(n_segs * 64)
        try:
            self._call("zkfhe_msm_segmented", bufs[0], points.shape[0], bufs[1], bufs[2], T, bufs[3], n_segs, dout)
            return dout.download(shape=(n_segs, 8))
        finally:
            for b in bufs + [dout]:
                if b is not None:
                    b.free()

    def witness_poly_mul_u64(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        n = a.size
        da, db, do = self.to_device(a), self.to_device(b), self.alloc((2 * n - 1) * 32)
        self._call("zkfhe_witness_poly_mul_u64", da, db, n, do)
        out = do.download(shape=(2 * n - 1, 4))
        da.free(), db.free(), do.free()
        return out

    def witness_div_mod(self, a, q):
        a = self._fr(a).reshape(-1, 4)
        n = a.shape[0]
        da, dd, dr = self.to_device(a), self.alloc(n * 32), self.alloc(n * 32)
        self._call("zkfhe_witness_div_mod", da, int(q), dd, dr, n)
        d, r = dd.download(shape=(n, 4)), dr.download(shape=(n, 4))
        da.free(), dd.free(), dr.free()
        return d, r

    def poly_mul_ternary_negacyclic(self, a, s, q):
        """zkfhe_poly_mul_ternary_negacyclic on host arrays: a of shape (N,) (shared) or (n_polys, N), s of shape (n_polys, N) with
        coefficients in {0, 1, q - 1}; returns a * s mod (x^N + 1, q), shape (n_polys, N).  A non-ternary s raises ZkfheError."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        s = np.ascontiguousarray(s, dtype=np.uint64)
        s2 = s.reshape(-1, s.shape[-1])
        n_polys, n = s2.shape
        a_count = 1 if a.ndim == 1 else a.shape[0]
        da, ds, do = self.to_device(a), self.to_device(s2), self.alloc(s2.nbytes)
        try:
            bad = ctypes.c_int()
            self._call("zkfhe_poly_mul_ternary_negacyclic", da, a_count, ds, n_polys, n, int(q), do, ctypes.byref(bad))
            return do.download(shape=(n_polys, n))
        finally:
            da.free(), ds.free(), do.free()
