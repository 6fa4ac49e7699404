"""Collective refresh and public collective key switching rates on the GPU (zkfhe_bfv_refresh_share, zkfhe_bfv_refresh_combine,
zkfhe_bfv_pcks_share, zkfhe_bfv_pcks_combine), with zkfhe_bfv_decrypt_share and zkfhe_bfv_decrypt_combine on the same batches for
comparison.  One JSON line per measurement:

  {"what": "refresh_share" | "pcks_share" | "decrypt_share", N, Q, cts, ms_per_call, cts_per_s, kernel_ms: {sample, rns_ntt, epilogue}}
  {"what": "refresh_combine" | "pcks_combine" | "decrypt_combine", N, Q, parties, cts, ms_per_call, cts_per_s, kernel_ms: {combine}}
  (refresh_combine also "sample": it regenerates a_j)

and, with --md, the tables of profiles/bfv_refresh.md on standard output after them.  Kernel times come from a separate profiled
pass.  Wall time is per call and includes the host checks and the copies of the inputs and outputs through pageable memory.

With --reuse-outputs the C entry points are called with output arrays that are allocated and touched once; without it the Python
methods allocate theirs on every call, and the first touch of those pages is part of the wall time.

    python tools/bfv_refresh_rate.py [--cts 2048] [--parties 3] [--reps 5] [--reuse-outputs] [--md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 536870909, 7), (4096, (1 << 60) - 93, 65537)]   # N, Q, T: the k = 13 parameters and a batching size


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


# the arguments of each C entry point (before its outputs) as the positional and keyword arguments of the Python method
PY_ARGS = {
    "refresh_share": lambda sk, crs, n, c1, seed, first, e: ((sk, crs, c1), dict(seed=seed, first_index=first, smudge_bound=e)),
    "pcks_share": lambda sk, pk0, pk1, n, c1, seed, first, e: ((sk, pk0, pk1, c1), dict(seed=seed, first_index=first, smudge_bound=e)),
    "decrypt_share": lambda sk, n, c1, seed, first, e: ((sk, c1), dict(seed=seed, first_index=first, smudge_bound=e)),
    "refresh_combine": lambda p, n, crs, first, c0, h0, h1: ((crs, c0, h0, h1), dict(first_index=first)),
    "pcks_combine": lambda p, n, c0, h0, h1: ((c0, h0, h1), {}),
    "decrypt_combine": lambda p, n, c0, d: ((c0, d), {}),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cts", type=int, default=2048)
    ap.add_argument("--parties", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reuse-outputs", action="store_true", help="call the C entry points with output arrays allocated once")
    ap.add_argument("--md", action="store_true", help="print the tables of profiles/bfv_refresh.md after the JSON lines")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    crs, count, p = os.urandom(32), a.cts, a.parties
    share_slots = (("sample", zk.PROF_BFV_SAMPLE), ("rns_ntt", zk.PROF_RNS_NTT), ("epilogue", zk.PROF_RNS_EPILOGUE))
    rows = []
    for n, q, t in SIZES:
        prm = (n, q, t, 19)
        sk = ctx.bfv_keygen_share(prm, crs, os.urandom(32))[0]
        _, pk0_to, pk1_to = ctx.bfv_fhe_keypair(prm, os.urandom(32))
        bound = (q // t // 2) // (4 * p)
        base = min(64, count)
        tile = lambda x: np.ascontiguousarray(np.tile(x, (-(-count // base), 1))[:count])  # noqa: E731
        c0 = tile(rng.integers(0, q, size=(base, n), dtype=np.uint64))   # the cost does not depend on the values
        c1 = tile(rng.integers(0, q, size=(base, n), dtype=np.uint64))
        h = np.ascontiguousarray(np.broadcast_to(c1, (p,) + c1.shape))
        seed = os.urandom(32)
        # (name, the C entry point's arguments before the outputs, the number of outputs, slots)
        calls = (
            ("refresh_share", (sk, crs, count, c1, seed, 0, bound), 2, share_slots),
            ("pcks_share", (sk, pk0_to, pk1_to, count, c1, seed, 0, bound), 2, share_slots),
            ("decrypt_share", (sk, count, c1, seed, 0, bound), 1, share_slots),
            ("refresh_combine", (p, count, crs, 0, c0, h, h), 2, (("sample", zk.PROF_BFV_SAMPLE), ("combine", zk.PROF_BFV_REFRESH_COMBINE))),
            ("pcks_combine", (p, count, c0, h, h), 2, (("combine", zk.PROF_BFV_PCKS_COMBINE),)),
            ("decrypt_combine", (p, count, c0, h), 1, (("combine", zk.PROF_BFV_DECRYPT_COMBINE),)),
        )
        for what, args, n_out, slots in calls:
            if a.reuse_outputs:   # output arrays allocated and touched once, as a C caller with buffers of its own would
                outs = [np.zeros((count, n), dtype=np.uint64) for _ in range(n_out)]
                run = lambda: ctx._call("zkfhe_bfv_" + what, prm, *args, *outs)  # noqa: E731
            else:                 # the Python methods: every call allocates its outputs
                method, margs = getattr(ctx, "bfv_" + what), PY_ARGS[what](*args)
                run = lambda: method(prm, *margs[0], **margs[1])  # noqa: E731
            ms = timed(run, a.reps)
            row = {"what": what, "N": n, "Q": q, "cts": count, "reuse_outputs": a.reuse_outputs, "ms_per_call": round(ms, 3),
                   "cts_per_s": round(count * 1e3 / ms, 1), "kernel_ms": kernels(ctx, run, slots)}
            if what.endswith("combine"):
                row["parties"] = p
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    if a.md:
        print("\n| N | Q | call | ciphertexts | wall ms / call | ciphertexts / s | kernel ms |\n|---|---|---|---|---|---|---|")
        for r in rows:
            kern = ", ".join("%s %.4f" % kv for kv in r["kernel_ms"].items())
            print("| %d | %d | `zkfhe_bfv_%s` | %d | %.3f | %d | %s |" % (r["N"], r["Q"], r["what"], r["cts"], r["ms_per_call"], r["cts_per_s"], kern))


if __name__ == "__main__":
    main()
