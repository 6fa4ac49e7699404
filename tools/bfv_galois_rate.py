"""BFV slot and rotation rates on the GPU (zkfhe_bfv_encode_slots, zkfhe_bfv_decode_slots, zkfhe_bfv_apply_galois, zkfhe_bfv_slot_sum)
and writes profiles/bfv_galois.md.  One JSON line per measurement on stdout:

  {"what": "encode" | "decode", N, Q, T, polys, ms_per_call, kernel_ms: {slot_ntt}}
  {"what": "apply_galois" | "slot_sum", N, Q, T, w, cts, ms_per_call, kernel_ms: {galois, rns_ntt}}

Kernel times come from a separate profiled pass (zkfhe_prof_* slots 6, 14 and 15).  Wall time is per call and includes the host
checks and the copies of the inputs and outputs through pageable memory.

    python tools/bfv_galois_rate.py [--cts 1,64] [--reps 5] [--out profiles/bfv_galois.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, (1 << 60) - 93, 12289), (4096, (1 << 60) - 93, 65537), (16384, (1 << 60) - 93, 65537)]   # N, Q, T
W = 16


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
    ap.add_argument("--cts", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_galois.md"))
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    counts = [int(x) for x in a.cts.split(",")]
    rows = []
    for n, q, t in SIZES:
        prm = (n, q, t, 19)
        sk = ctx.bfv_fhe_keypair(prm, os.urandom(32))[0]
        elements = zk.bfv_slot_sum_elements(prm)
        keys = [ctx.bfv_galois_keygen(prm, sk, g, base_bits=W) for g in elements]
        gk0, gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
        for count in counts:
            v = rng.integers(0, t, size=(count, n), dtype=np.uint64)
            m = ctx.bfv_encode_slots(prm, v)
            for what, fn in (("encode", lambda: ctx.bfv_encode_slots(prm, v)), ("decode", lambda: ctx.bfv_decode_slots(prm, m))):
                ms = timed(fn, a.reps)
                kern = kernels(ctx, fn, (("slot_ntt", zk.PROF_BFV_SLOT_NTT),))
                rows.append(dict(what=what, N=n, Q=q, T=t, polys=count, ms_per_call=round(ms, 3), kernel_ms=kern))
                print(json.dumps(rows[-1]), flush=True)
            c0 = rng.integers(0, q, size=(count, n), dtype=np.uint64)   # the cost does not depend on the values
            c1 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
            calls = (("apply_galois", lambda: ctx.bfv_apply_galois(prm, c0, c1, elements[0], gk0[0], gk1[0], base_bits=W)),
                     ("slot_sum", lambda: ctx.bfv_slot_sum(prm, c0, c1, gk0, gk1, base_bits=W)))
            for what, fn in calls:
                ms = timed(fn, a.reps)
                kern = kernels(ctx, fn, (("galois", zk.PROF_BFV_GALOIS), ("rns_ntt", zk.PROF_RNS_NTT)))
                rows.append(dict(what=what, N=n, Q=q, T=t, w=W, cts=count, ms_per_call=round(ms, 3), kernel_ms=kern))
                print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    qs = lambda q: "2^60 − 93" if q == (1 << 60) - 93 else str(q)  # noqa: E731
    lines = ["# BFV slots and rotations on the GPU (`zkfhe_bfv_encode_slots`, `zkfhe_bfv_decode_slots`, `zkfhe_bfv_apply_galois`, "
             "`zkfhe_bfv_slot_sum`)", "",
             "One MI355X.  `python tools/bfv_galois_rate.py --reps %d` (%d timed calls per row after one warm-up).  Wall time is per "
             "call and includes the host range checks and the copies of inputs and outputs through pageable host memory.  Kernel "
             "time comes from a separate profiled pass (`zkfhe_prof_*` slots 6, 14 and 15).  B = 19, w = %d.  Every call "
             "transforms its Galois keys once (the RNS NTT column: the keys' transforms; `slot_sum` transforms all log2(N) keys)."
             % (a.reps, a.reps, W), "",
             "## Encode and decode (one LDS NTT mod T per polynomial)", "",
             "| N | T | polynomials | encode wall ms | encode kernel ms | decode wall ms | decode kernel ms |", "|---|---|---|---|---|---|---|"]
    for n, q, t in SIZES:
        for count in counts:
            e = next(r for r in rows if r["what"] == "encode" and r["N"] == n and r["polys"] == count)
            d = next(r for r in rows if r["what"] == "decode" and r["N"] == n and r["polys"] == count)
            lines.append("| %d | %d | %d | %.3f | %.4f | %.3f | %.4f |" % (n, t, count, e["ms_per_call"], e["kernel_ms"]["slot_ntt"],
                                                                        d["ms_per_call"], d["kernel_ms"]["slot_ntt"]))
    lines += ["", "## Key switches", "",
              "`apply_galois` is one rotation (g = 5); `slot_sum` is log2(N) rotations and additions on device buffers.", "",
              "| N | Q | T | call | ciphertexts | wall ms / call | key switch + epilogue ms | RNS NTT ms (keys) |", "|---|---|---|---|---|---|---|---|"]
    for n, q, t in SIZES:
        for what in ("apply_galois", "slot_sum"):
            for count in counts:
                r = next(r for r in rows if r["what"] == what and r["N"] == n and r["cts"] == count)
                lines.append("| %d | %s | %d | `%s` | %d | %.3f | %.4f | %.4f |" % (n, qs(q), t, what, count, r["ms_per_call"],
                                                                                  r["kernel_ms"]["galois"], r["kernel_ms"]["rns_ntt"]))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
