"""BFV evaluation rate on the GPU (zkfhe_bfv_sum, zkfhe_bfv_mul).  One JSON line per measurement:

  {"what": "sum", N, Q, cts, ms_per_call, cts_per_s, kernel_ms: {sum}}                                   (kernels: a separate profiled pass)
  {"what": "mul", N, Q, w, pairs, ms_per_call, mul_per_s, kernel_ms: {rns_ntt, tensor, relin, epilogue}}

Wall time is per call and includes the host checks and the copies of the inputs and outputs through pageable memory.

    python tools/bfv_eval_rate.py [--sums 64,4096] [--pairs 1,8,64] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 536870909, 7, 8), (4096, (1 << 60) - 93, 65537, 16), (16384, (1 << 60) - 93, 65537, 16)]   # N, Q, T, base_bits


def timed(fn, reps):
    fn()   # warm-up: tables, arena
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def kernels(ctx, fn, slots):
    ctx.prof_enable(True)   # resets the counters
    fn()
    out = {name: round(ctx.prof_read(slot)["total_ms"], 4) for name, slot in slots}
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sums", default="64,4096")
    ap.add_argument("--pairs", default="1,8,64")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    sums = [int(x) for x in a.sums.split(",")]
    pairs = [int(x) for x in a.pairs.split(",")]
    for n, q, t, w in SIZES:
        prm = (n, q, t, 19)
        sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
        rlk0, rlk1 = ctx.bfv_relin_keygen(prm, sk, os.urandom(32), base_bits=w)
        base = max(64, 2 * max(pairs))
        m = np.array([int(x) % q for x in rng.integers(-(t // 2), t // 2 + 1, base * n)], dtype=np.uint64).reshape(base, n)
        ct = ctx.bfv_encrypt(prm, pk0, pk1, m)
        for count in sums:   # the encryptions repeated: the sum's cost does not depend on the values
            c0 = np.ascontiguousarray(np.tile(ct["c0"], (-(-count // base), 1))[:count])
            c1 = np.ascontiguousarray(np.tile(ct["c1"], (-(-count // base), 1))[:count])
            run = lambda: ctx.bfv_sum(prm, c0, c1)  # noqa: E731
            ms = timed(run, a.reps)
            kern = kernels(ctx, run, (("sum", zk.PROF_BFV_ELEMENTWISE),))
            print(json.dumps({"what": "sum", "N": n, "Q": q, "cts": count, "ms_per_call": round(ms, 3),
                              "cts_per_s": round(count * 1e3 / ms, 1), "kernel_ms": kern}), flush=True)
        for p in pairs:
            a0, a1, b0, b1 = ct["c0"][:p], ct["c1"][:p], ct["c0"][p:2 * p], ct["c1"][p:2 * p]
            run = lambda: ctx.bfv_mul(prm, a0, a1, b0, b1, rlk0, rlk1, base_bits=w)  # noqa: E731
            ms = timed(run, a.reps)
            kern = kernels(ctx, run, (("rns_ntt", zk.PROF_RNS_NTT), ("tensor", zk.PROF_BFV_TENSOR), ("relin", zk.PROF_BFV_RELIN),
                                      ("epilogue", zk.PROF_BFV_EVAL_EPILOGUE)))
            print(json.dumps({"what": "mul", "N": n, "Q": q, "w": w, "pairs": p, "ms_per_call": round(ms, 3),
                              "mul_per_s": round(p * 1e3 / ms, 1), "kernel_ms": kern}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
