"""The G1 FFT (zkfhe_g1_fft, inverse) against what a user could assemble from the calls the library had before it, in one process,
and the wall time of the ceremony calls at k = 13.

  fused     zkfhe_g1_fft(inverse): one launch per stage, points in the accumulator form between the stages.
  composed  the same radix-2 schedule stage by stage: one zkfhe_g1_mul over the n/2 twiddled operands and two zkfhe_g1_add, affine
            in and out of every call (two field inversions per point and stage).  The operands are gathered and scattered, and t is
            negated, with torch on the same stream; index lists and per-stage twiddles are made before the clock starts.  The stage
            of twiddle 1 skips its multiplication and the last stage carries the n^-1, as in the fused call.
Both results are compared byte for byte before anything is timed.  Per size: minimum of --reps after a warm-up, the two paths
alternating.  One JSON line per size, then one for the ceremony calls.

    python tools/srs_fft_rate.py [--sizes 13,16,19] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="13,16,19")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ceremony", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("ZKFHE_TABLE_GB", "4")
    import torch
    import zk_fhe_amd as zk
    from oracle import binding as orc
    from oracle import pyref
    stream = torch.cuda.Stream()
    ctx = zk.Context(0, stream=stream.cuda_stream)
    lib = ctx.lib
    dev = torch.device("cuda:0")
    vp = ctypes.c_void_p

    def M(v):
        return orc.ints_to_mont([v % pyref.R])[0]

    def to_dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)

    q_limbs = torch.tensor([(Q >> (32 * i)) & 0xffffffff for i in range(8)], dtype=torch.int64, device=dev)

    def negate(pts):
        """(m, 8) int64 affine Montgomery points -> their negatives: y -> p - y on 32-bit limbs, the identity (0, 0) stays"""
        y = pts[:, 4:].contiguous().view(torch.int32).to(torch.int64) & 0xffffffff   # (m, 8) limbs
        out = torch.empty_like(y)
        borrow = torch.zeros(y.shape[0], dtype=torch.int64, device=dev)
        for i in range(8):
            d = q_limbs[i] - y[:, i] - borrow
            borrow = (d < 0).to(torch.int64)
            out[:, i] = d & 0xffffffff
        ny = out[:, 0::2] | (out[:, 1::2] << 32)
        zero = (pts[:, 4:] == 0).all(dim=1, keepdim=True)
        res = pts.clone()
        res[:, 4:] = torch.where(zero, pts[:, 4:], ny)
        return res

    gen = orc.points_to_arr([pyref.G1_GEN])[0]
    rng = np.random.default_rng(19)
    with torch.cuda.stream(stream):
        for log_n in [int(s) for s in a.sizes.split(",")]:
            n, h = 1 << log_n, 1 << (log_n - 1)
            # random points, made on the GPU
            k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
            k[:, 3] &= np.uint64((1 << 60) - 1)
            pts_host = ctx.g1_mul(np.repeat(gen[None], n, axis=0), k)
            pts = to_dev(pts_host)
            w_inv = pow(pyref.root_of_unity(log_n), -1, pyref.R)
            tw = orc.fr_powers(M(1), M(w_inv), n)
            n_inv = M(pow(n, -1, pyref.R))
            rev = np.array([int(format(i, "0%db" % log_n)[::-1], 2) for i in range(n)], dtype=np.int64)
            rev_d = torch.from_numpy(rev).to(dev)
            stages = []
            for s in range(log_n):
                half, blocks = 1 << s, h >> s
                t = np.arange(h, dtype=np.int64)
                j, blk = t & (half - 1), t >> s
                lo = (blk << (s + 1)) + j
                tws = tw[j << (log_n - 1 - s)]
                last = s == log_n - 1
                if last:
                    tws = orc.fr_scale(tws, n_inv)
                stages.append((torch.from_numpy(lo).to(dev), torch.from_numpy(lo + half).to(dev), None if s == 0 and not last else to_dev(tws),
                               to_dev(np.repeat(n_inv[None], h, axis=0)) if last else None))

            def p(t):
                return vp(t.data_ptr())

            def composed():
                x = torch.empty_like(pts)
                x[rev_d] = pts
                for lo, hi, tws, scale in stages:
                    b = x[hi].contiguous()
                    al = x[lo].contiguous()
                    if tws is not None:
                        ctx._check(lib.zkfhe_g1_mul(ctx.h, p(b), p(tws), p(b), h))
                    if scale is not None:
                        ctx._check(lib.zkfhe_g1_mul(ctx.h, p(al), p(scale), p(al), h))
                    nb = negate(b)
                    s_, d_ = torch.empty_like(al), torch.empty_like(al)
                    ctx._check(lib.zkfhe_g1_add(ctx.h, p(al), p(b), p(s_), h))
                    ctx._check(lib.zkfhe_g1_add(ctx.h, p(al), p(nb), p(d_), h))
                    x[lo] = s_
                    x[hi] = d_
                stream.synchronize()
                return x

            def fused():
                x = pts.clone()
                ctx._check(lib.zkfhe_g1_fft(ctx.h, p(x), log_n, 1))   # waits
                return x

            assert torch.equal(fused(), composed()), "the composed path and zkfhe_g1_fft differ at log_n = %d" % log_n
            best = {"fused": float("inf"), "composed": float("inf")}
            for _ in range(a.reps):
                for name, fn in (("fused", fused), ("composed", composed)):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    best[name] = min(best[name], time.perf_counter() - t0)
            ctx.prof_enable(True)
            fused()
            pr = ctx.prof_read(zk.PROF_G1_FFT)
            ctx.prof_enable(False)
            print(json.dumps({"log_n": log_n, "fused_ms": round(best["fused"] * 1e3, 3), "composed_ms": round(best["composed"] * 1e3, 3),
                              "composed_over_fused": round(best["composed"] / best["fused"], 3), "butterfly_kernels_ms": round(pr["total_ms"], 3),
                              "scalar_multiplications": int(pr["ops"]), "reps": a.reps}), flush=True)
            del pts, stages
        if not a.no_ceremony:
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "k13.srs")
                srs = zk.Srs(ctx, 13)
                srs.save(path)
                srs.destroy()
                blob = open(path, "rb").read()
                g = np.frombuffer(blob, dtype=np.uint64, count=8 << 13, offset=4).reshape(-1, 8).copy()
                gl = np.frombuffer(blob, dtype=np.uint64, count=8 << 13, offset=4 + (64 << 13)).reshape(-1, 8).copy()
                res = {}
                for rep in range(3):
                    t0 = time.perf_counter()
                    srs = zk.Srs.load_downsized(ctx, path, 13)
                    res["load_downsized_ms"] = min(res.get("load_downsized_ms", 1e30), (time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    assert srs.check(bytes(32)) == 0
                    res["check_ms"] = min(res.get("check_ms", 1e30), (time.perf_counter() - t0) * 1e3)
                    srs.destroy()
                    t0 = time.perf_counter()
                    srs = zk.Srs.from_points(ctx, 13, g, gl)
                    res["from_points_ms"] = min(res.get("from_points_ms", 1e30), (time.perf_counter() - t0) * 1e3)
                    srs.destroy()
                    t0 = time.perf_counter()
                    ctx.g1_fft(g, inverse=True)
                    res["g1_fft_with_copies_ms"] = min(res.get("g1_fft_with_copies_ms", 1e30), (time.perf_counter() - t0) * 1e3)
                    # k = 3: eight points, so the call is the host pairing and fixed costs
                    small = zk.Srs(ctx, 3)
                    t0 = time.perf_counter()
                    assert small.check(bytes(32)) == 0
                    res["check_k3_ms"] = min(res.get("check_k3_ms", 1e30), (time.perf_counter() - t0) * 1e3)
                    small.destroy()
                print(json.dumps({"k": 13, **{key: round(v, 2) for key, v in res.items()}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
