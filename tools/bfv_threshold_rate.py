"""Threshold BFV rate on the GPU (zkfhe_bfv_decrypt_share, zkfhe_bfv_decrypt_combine), with zkfhe_bfv_decrypt on the same batches for
comparison.  One JSON line per measurement:

  {"what": "share", N, Q, cts, ms_per_call, cts_per_s, kernel_ms: {sample, rns_ntt, epilogue}}
  {"what": "combine", N, Q, parties, cts, ms_per_call, cts_per_s, kernel_ms: {combine}}
  {"what": "decrypt", N, Q, cts, ms_per_call, cts_per_s, kernel_ms: {rns_ntt, epilogue}}

Kernel times come from a separate profiled pass.  Wall time is per call and includes the host checks and the copies of the inputs
and outputs through pageable memory.

    python tools/bfv_threshold_rate.py [--cts 1,64,4096] [--parties 3,16] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 536870909, 7), (4096, (1 << 60) - 93, 65537), (16384, (1 << 60) - 93, 65537)]   # N, Q, T


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
    ap.add_argument("--cts", default="1,64,4096")
    ap.add_argument("--parties", default="3,16")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    counts = [int(x) for x in a.cts.split(",")]
    parties = [int(x) for x in a.parties.split(",")]
    crs = os.urandom(32)
    for n, q, t in SIZES:
        prm = (n, q, t, 19)
        sk = ctx.bfv_keygen_share(prm, crs, os.urandom(32))[0]
        bound = (q // t // 2) // max(parties) - 1
        base = min(64, max(counts))
        c0b = rng.integers(0, q, size=(base, n), dtype=np.uint64)   # the cost does not depend on the values
        c1b = rng.integers(0, q, size=(base, n), dtype=np.uint64)
        for count in counts:
            c0 = np.ascontiguousarray(np.tile(c0b, (-(-count // base), 1))[:count])
            c1 = np.ascontiguousarray(np.tile(c1b, (-(-count // base), 1))[:count])
            seed = os.urandom(32)
            run = lambda: ctx.bfv_decrypt_share(prm, sk, c1, seed=seed, smudge_bound=bound)  # noqa: E731
            ms = timed(run, a.reps)
            kern = kernels(ctx, run, (("sample", zk.PROF_BFV_SAMPLE), ("rns_ntt", zk.PROF_RNS_NTT), ("epilogue", zk.PROF_RNS_EPILOGUE)))
            print(json.dumps({"what": "share", "N": n, "Q": q, "cts": count, "ms_per_call": round(ms, 3),
                              "cts_per_s": round(count * 1e3 / ms, 1), "kernel_ms": kern}), flush=True)
            run = lambda: ctx.bfv_decrypt(prm, sk, c0, c1)  # noqa: E731
            ms = timed(run, a.reps)
            kern = kernels(ctx, run, (("rns_ntt", zk.PROF_RNS_NTT), ("epilogue", zk.PROF_RNS_EPILOGUE)))
            print(json.dumps({"what": "decrypt", "N": n, "Q": q, "cts": count, "ms_per_call": round(ms, 3),
                              "cts_per_s": round(count * 1e3 / ms, 1), "kernel_ms": kern}), flush=True)
            for p in parties:
                d = np.ascontiguousarray(np.broadcast_to(c1, (p,) + c1.shape))
                run = lambda: ctx.bfv_decrypt_combine(prm, c0, d)  # noqa: E731
                ms = timed(run, a.reps)
                kern = kernels(ctx, run, (("combine", zk.PROF_BFV_DECRYPT_COMBINE),))
                print(json.dumps({"what": "combine", "N": n, "Q": q, "parties": p, "cts": count, "ms_per_call": round(ms, 3),
                                  "cts_per_s": round(count * 1e3 / ms, 1), "kernel_ms": kern}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
