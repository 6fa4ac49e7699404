"""Rates of the encrypted matrix-vector product on the GPU: zkfhe_bfv_linear_transform against the same transform composed from the
calls that were there before it.  One JSON line per measurement on stdout:

  {"mode": "new" | "composition", N, Q, T, w, K, cts, ms_per_call, kernel_ms: {name: ms}, [acc_bytes]}

  --mode new           one zkfhe_bfv_linear_transform call per transform
  --mode composition   K x zkfhe_bfv_apply_galois, K x zkfhe_bfv_mul_plain, K - 1 x zkfhe_bfv_add.  This mode uses no symbol newer
                       than those, so it also runs against a build of an earlier commit (copy this file into that tree's tools/).
  --report A.jsonl ... reads the lines of earlier runs (in the order given: new and composition runs alternating) and writes
                       the table of profiles/bfv_linear.md to --out (or stdout)

Kernel times come from a separate profiled pass (every zkfhe_prof_* slot of the BFV layer).  Wall time is per transform and includes
the host checks and the copies of inputs and outputs through pageable memory.  K distinct rotations g = 5^(k+1), none of them 1.

    python tools/bfv_linear_rate.py --mode new [--reps 10] > new.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q60 = (1 << 60) - 93
SIZES = [(1024, Q60, 12289), (4096, Q60, 65537), (16384, Q60, 65537)]   # N, Q, T
ELEMENTS = (2, 8, 32)
CTS = (1, 64)
W = 8
BFV_SLOTS = range(5, 16)   # the BFV slots that exist in both builds
NAMES = {6: "rns_ntt", 10: "epilogue", 11: "elementwise", 14: "galois", 16: "hoist", 17: "accumulate"}


def timed(fn, reps):
    fn()   # warm-up: tables, arena
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()   # every call waits for its result
    return (time.perf_counter() - t0) * 1e3 / reps


def kernels(ctx, fn, slots):
    ctx.prof_enable(True)   # resets the counters
    fn()
    out = {s: ctx.prof_read(s) for s in slots}
    ctx.prof_enable(False)
    return out


def measure(mode, reps):
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    slots = list(BFV_SLOTS) + ([16, 17] if mode == "new" else [])
    for n, q, t in SIZES:
        prm = (n, q, t, 19)
        sk = ctx.bfv_fhe_keypair(prm, os.urandom(32))[0]
        elements = [pow(5, k + 1, 2 * n) for k in range(max(ELEMENTS))]
        keys = [ctx.bfv_galois_keygen(prm, sk, g, base_bits=W) for g in elements]
        gk0, gk1 = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
        diag = np.array([[int(x) % q for x in row] for row in rng.integers(-(t // 2), t // 2 + 1, size=(max(ELEMENTS), n))], dtype=np.uint64)
        for count in CTS:
            c0 = rng.integers(0, q, size=(count, n), dtype=np.uint64)   # the cost does not depend on the values
            c1 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
            for K in ELEMENTS:
                if mode == "new":
                    def fn():
                        return ctx.bfv_linear_transform(prm, c0, c1, elements[:K], gk0[:K], gk1[:K], diag[:K], base_bits=W)
                else:
                    def fn():
                        acc = None
                        for k in range(K):
                            r0, r1 = ctx.bfv_apply_galois(prm, c0, c1, elements[k], gk0[k], gk1[k], base_bits=W)
                            p0, p1 = ctx.bfv_mul_plain(prm, r0, r1, diag[k])
                            acc = (p0, p1) if acc is None else ctx.bfv_add(prm, acc[0], acc[1], p0, p1)
                        return acc
                ms = timed(fn, reps)
                prof = kernels(ctx, fn, slots)
                row = dict(mode=mode, N=n, Q=q, T=t, w=W, K=K, cts=count, ms_per_call=round(ms, 3),
                           kernel_ms={NAMES.get(s, str(s)): round(p["total_ms"], 4) for s, p in prof.items() if p["launches"]})
                if mode == "new":
                    row["acc_bytes"] = prof[17]["algorithmic_bytes"]
                print(json.dumps(row), flush=True)
    ctx.close()


def report(files, out):
    runs = [[json.loads(line) for line in open(f) if line.startswith("{")] for f in files]
    by_mode = {m: [r for r in runs if r and r[0]["mode"] == m] for m in ("new", "composition")}

    def cell(rows, n, K, count, get):
        return " / ".join(get(next(x for x in r if x["N"] == n and x["K"] == K and x["cts"] == count)) for r in rows)

    total = lambda x: "%.3f" % sum(x["kernel_ms"].values())  # noqa: E731
    lines = ["| N | K | ciphertexts | wall ms new | wall ms composition | composition / new | kernel ms new | kernel ms composition | "
             "accumulate ms | accumulate share of kernel time | accumulate GB/s |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, _, _ in SIZES:
        for K in ELEMENTS:
            for count in CTS:
                new = [next(x for x in r if x["N"] == n and x["K"] == K and x["cts"] == count) for r in by_mode["new"]]
                comp = [next(x for x in r if x["N"] == n and x["K"] == K and x["cts"] == count) for r in by_mode["composition"]]
                ratio = min(c["ms_per_call"] for c in comp) / max(x["ms_per_call"] for x in new)   # the least favourable pairing
                acc = [x["kernel_ms"].get("accumulate", 0.0) for x in new]
                lines.append("| %d | %d | %d | %s | %s | %.2f | %s | %s | %s | %s | %s |" % (
                    n, K, count, cell(by_mode["new"], n, K, count, lambda x: "%.3f" % x["ms_per_call"]),
                    cell(by_mode["composition"], n, K, count, lambda x: "%.3f" % x["ms_per_call"]), ratio,
                    cell(by_mode["new"], n, K, count, total), cell(by_mode["composition"], n, K, count, total),
                    " / ".join("%.4f" % a for a in acc),
                    " / ".join("%.0f %%" % (100 * a / sum(x["kernel_ms"].values())) for a, x in zip(acc, new)),
                    " / ".join("%.0f" % (x["acc_bytes"] / (a * 1e6)) if a else "-" for a, x in zip(acc, new))))
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("new", "composition"), default="new")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--report", nargs="+", help="JSON-line files of earlier runs")
    ap.add_argument("--out", help="where --report writes its table (default: stdout)")
    a = ap.parse_args()
    if a.report:
        report(a.report, a.out)
    else:
        measure(a.mode, a.reps)


if __name__ == "__main__":
    main()
