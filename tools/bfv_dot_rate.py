"""Fused BFV inner products on the GPU (zkfhe_bfv_dot, zkfhe_bfv_dot_plain) against the composition that gives the same tally
(zkfhe_bfv_mul or zkfhe_bfv_mul_plain on n pairs, then zkfhe_bfv_sum), in one process on the same inputs.  One JSON line per row:

  {"what": "dot" | "dot_plain", N, Q, w, terms, fused: {ms_per_call, kernel_ms, kernels: {...}}, composed: {...}, same_result}

Wall time is per call and includes the host checks and the copies of the inputs and outputs through pageable memory; the fused
and the composed call alternate inside the timed loop.  Kernel time is the sum of the library's profiling slots over one separate
profiled call each.  same_result: dot_plain equals the composition bit for bit; dot differs from it in the roundings only, so the
row reports whether both decrypt to the same plaintext (they need not where the repeated terms use up the noise budget: the tool
times the calls, it does not choose parameters for the sum).

    python tools/bfv_dot_rate.py [--terms 8,64,512] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 536870909, 7, 8), (4096, (1 << 60) - 93, 65537, 16), (16384, (1 << 60) - 93, 65537, 16)]   # N, Q, T, base_bits
BASE = 128   # fresh encryptions per size; longer vectors repeat them (the cost does not depend on the values)


def timed_pair(f, g, reps):
    """ms per call of f and of g, alternating after one warm-up each (tables, arena)"""
    f(), g()
    tf = tg = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t1 = time.perf_counter()
        g()
        tf, tg = tf + t1 - t0, tg + time.perf_counter() - t1
    return tf * 1e3 / reps, tg * 1e3 / reps


def kernels(ctx, zk, fn):
    slots = (("rns_ntt", zk.PROF_RNS_NTT), ("dot", zk.PROF_BFV_DOT), ("tensor", zk.PROF_BFV_TENSOR), ("relin", zk.PROF_BFV_RELIN),
             ("epilogue", zk.PROF_BFV_EVAL_EPILOGUE), ("elementwise", zk.PROF_BFV_ELEMENTWISE))
    ctx.prof_enable(True)   # resets the counters
    fn()
    out = {name: round(ctx.prof_read(slot)["total_ms"], 4) for name, slot in slots}
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--terms", default="8,64,512")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    for n, q, t, w in SIZES:
        prm = (n, q, t, 19)
        sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
        rlk0, rlk1 = ctx.bfv_relin_keygen(prm, sk, os.urandom(32), base_bits=w)
        m = rng.integers(-(t // 2), t // 2 + 1, (2 * BASE, n))
        m = np.where(m < 0, m + q, m).astype(np.uint64)
        ct = ctx.bfv_encrypt(prm, pk0, pk1, m)
        for terms in [int(x) for x in a.terms.split(",")]:
            rep = lambda x: np.ascontiguousarray(np.tile(x, (-(-terms // BASE), 1))[:terms])  # noqa: E731
            a0, a1, b0, b1 = rep(ct["c0"][:BASE]), rep(ct["c1"][:BASE]), rep(ct["c0"][BASE:]), rep(ct["c1"][BASE:])
            p = rep(m[BASE:])
            cases = (
                ("dot", lambda: ctx.bfv_dot(prm, a0, a1, b0, b1, rlk0, rlk1, base_bits=w),
                 lambda: ctx.bfv_sum(prm, *ctx.bfv_mul(prm, a0, a1, b0, b1, rlk0, rlk1, base_bits=w))),
                ("dot_plain", lambda: ctx.bfv_dot_plain(prm, a0, a1, p), lambda: ctx.bfv_sum(prm, *ctx.bfv_mul_plain(prm, a0, a1, p))),
            )
            for what, fused, composed in cases:
                x, y = fused(), composed()
                if what == "dot":
                    same = bool(np.array_equal(ctx.bfv_decrypt(prm, sk, *x), ctx.bfv_decrypt(prm, sk, *y)))
                else:
                    same = bool(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]))
                ms_f, ms_c = timed_pair(fused, composed, a.reps)
                kf, kc = kernels(ctx, zk, fused), kernels(ctx, zk, composed)
                print(json.dumps({"what": what, "N": n, "Q": q, "w": w, "terms": terms,
                                  "fused": {"ms_per_call": round(ms_f, 3), "kernel_ms": round(sum(kf.values()), 4), "kernels": kf},
                                  "composed": {"ms_per_call": round(ms_c, 3), "kernel_ms": round(sum(kc.values()), 4), "kernels": kc},
                                  "same_result": same}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
