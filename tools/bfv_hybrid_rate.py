"""Hybrid key switching (zkfhe_bfv_evk_create_hybrid) beside the ordinary key switch of a resident key set: noise and time.

Noise: the table of profiles/bfv_pack.md again.  Fresh encryptions of random plaintexts go through zkfhe_bfv_cts_apply_galois_evk
(g = 5), zkfhe_bfv_cts_slot_sum and zkfhe_bfv_cts_pack (n = 1, 64, 1024 at random positions) with an ordinary key set and with hybrid
sets for a 30-bit P and for the largest admissible P coprime to Q; zkfhe_bfv_noise of each result (the largest of the batch) stands
beside floor(Q/T)/2.  A pack must also decrypt to the expected placement.
Time: pack (n = 64, 1024) and apply_galois (64 ciphertexts) with the hybrid set (30-bit P) beside the ordinary set at equal (w, l).
After a warm-up of both the two alternate; wall time is around the whole call, which waits for its result; kernel time is the sum of
every profiling slot, from profiled passes of their own.  Both are the median with the lowest and the highest repeat.  Then the row
the feature is for: per n the widest w whose hybrid noise stays below the ordinary w = 4 noise of the same n, with both times.

One JSON line per point, then the markdown of profiles/bfv_hybrid.md, written to --out.

    python tools/bfv_hybrid_rate.py [--reps 5] [--prof-reps 3] [--out profiles/bfv_hybrid.md] [--asm FILE]

--asm FILE appends the output of tools/device_asm_diff.py (parent against this commit, made without a GPU) as a section of its own.
--ordinary-only TAG times the ordinary legs alone and tags its JSON lines: with --package-root DIR (where a built checkout's
zk_fhe_amd.py lies) the same tool measures the parent commit, whose runs alternate with this commit's in one session; the markdown
then says per row whether this commit's lowest-to-highest range overlaps the parent's.
--from-rows FILE renders the markdown again from the JSON lines of an earlier run (--device names its device) and needs no GPU.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q29 = 536870909
Q60 = (1 << 60) - 93
K13 = (1024, Q29, 7, 19)
P4096 = (4096, Q60, 65537, 19)
P30 = (1 << 30) - 35
WIDTHS = [(K13, 4), (K13, 8), (K13, 16), (K13, 29), (P4096, 8), (P4096, 16), (P4096, 32)]
PACK_N = (1, 64, 1024)
TIMED = [(K13, 4), (K13, 8), (K13, 16), (K13, 29), (P4096, 16)]
KINDS = ("ordinary", "hybrid P30", "hybrid P max")


def pack_elements(n_ring):
    return [(1 << l) + 1 for l in range(1, n_ring.bit_length())]


def key_sets(ctx, zk, np, prm, w, hybrid=True):
    """one secret key; its ordinary set and (hybrid) its two hybrid sets over the slot-sum and pack elements"""
    sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
    elements = sorted(set(int(g) for g in zk.bfv_slot_sum_elements(prm)) | set(pack_elements(prm[0])))
    ks = [ctx.bfv_galois_keygen(prm, sk, g, base_bits=w) for g in elements]
    sets = {"ordinary": ctx.bfv_evk(prm, w, None, elements, np.array([k[0] for k in ks]), np.array([k[1] for k in ks]))}
    if not hybrid:
        return sk, pk0, pk1, sets, 0
    top = zk.bfv_hybrid_max_p(prm, w)
    while math.gcd(top, prm[1]) != 1:
        top -= 1
    for kind, p in (("hybrid P30", P30), ("hybrid P max", top)):
        ks = [ctx.bfv_galois_keygen_hybrid(prm, p, sk, g, base_bits=w) for g in elements]
        sets[kind] = ctx.bfv_evk_hybrid(prm, p, w, elements=elements, gk=tuple(np.array([k[j] for k in ks]) for j in range(4)))
    return sk, pk0, pk1, sets, top


def fresh(ctx, np, prm, pk0, pk1, n, rng):
    n_ring, q, t, _ = prm
    m = rng.integers(-(t // 2), t // 2 + 1, size=(n, n_ring))
    m = np.where(m < 0, m + q, m).astype(np.uint64)
    return m, ctx.bfv_encrypt(prm, pk0, pk1, m, os.urandom(32))


def noise_rows(ctx, zk, np, prm, w, keys, rng):
    n_ring, q, t, _ = prm
    sk, pk0, pk1, sets, top = keys
    base = {"N": n_ring, "Q": q, "T": t, "w": w, "l": zk.bfv_relin_digits(prm, w), "half_delta": (q // t) // 2, "p_max": top}
    rows = []
    m, ct = fresh(ctx, np, prm, pk0, pk1, 4, rng)
    with ctx.bfv_cts(prm, ct["c0"], ct["c1"]) as a:
        for op, call in (("apply_galois", lambda evk: a.apply_galois_evk(5, evk)), ("slot_sum", lambda evk: a.slot_sum(evk))):
            row = dict(base, op=op, n=4, fresh_noise=int(ctx.bfv_noise(prm, sk, ct["c0"], ct["c1"]).max()))
            for kind, evk in sets.items():
                with call(evk) as out:
                    row[kind] = int(ctx.bfv_noise(prm, sk, *out.download()).max())
            rows.append(row)
    for n in PACK_N:
        m, ct = fresh(ctx, np, prm, pk0, pk1, n, rng)
        pos = rng.integers(0, n_ring, size=n, dtype=np.uint64)
        want = np.zeros(n_ring, dtype=np.uint64)
        want[n_ring - 1 - np.arange(n) * (n_ring // n)] = m[np.arange(n), n_ring - 1 - pos.astype(np.int64)]
        row = dict(base, op="pack", n=n, fresh_noise=int(ctx.bfv_noise(prm, sk, ct["c0"], ct["c1"]).max()), decrypts={})
        with ctx.bfv_cts(prm, ct["c0"], ct["c1"]) as a:
            for kind, evk in sets.items():
                with a.pack(n, evk, pos=pos) as out:
                    o0, o1 = out.download()
                row[kind] = int(ctx.bfv_noise(prm, sk, o0, o1)[0])
                row["decrypts"][kind] = bool(np.array_equal(ctx.bfv_decrypt(prm, sk, o0, o1)[0], want))
        rows.append(row)
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def kernel_ms(ctx, zk, fn):
    ctx.prof_enable(True)   # resets the slots
    fn()
    prof = {s: ctx.prof_read(s) for s in range(zk.PROF_BFV_PACK + 1)}
    ctx.prof_enable(False)
    return sum(p["total_ms"] for p in prof.values())


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def time_rows(ctx, zk, np, prm, w, keys, reps, prof_reps, rng, kinds=("ordinary", "hybrid P30"), tag=None):
    n_ring, q = prm[0], prm[1]
    sk, pk0, pk1, sets, _ = keys
    rows = []
    for op, n in (("pack", 64), ("pack", 1024), ("apply_galois", 64)):
        a = ctx.bfv_cts(prm, rng.integers(0, q, size=(n, n_ring), dtype=np.uint64), rng.integers(0, q, size=(n, n_ring), dtype=np.uint64))
        out = ctx.bfv_cts_zeros(prm, 1 if op == "pack" else n)
        legs = {kind: (lambda evk=sets[kind]: a.pack(n, evk, out=out) if op == "pack" else a.apply_galois_evk(5, evk, out=out))
                for kind in kinds}
        row = {"commit": tag, "time": op, "N": n_ring, "Q": q, "w": w, "l": zk.bfv_relin_digits(prm, w), "n": n}
        try:
            for fn in legs.values():
                fn()   # warm-up: tables, arena, code objects
            wall, kern = {k: [] for k in legs}, {k: [] for k in legs}
            for _ in range(reps):
                for name, fn in legs.items():   # A/B
                    t0 = time.perf_counter()
                    fn()   # waits for its result
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            for _ in range(prof_reps):
                for name, fn in legs.items():
                    kern[name].append(kernel_ms(ctx, zk, fn))
            for name in legs:
                row[name] = {"wall_ms": stats(wall[name]), "kernel_ms": stats(kern[name])}
        finally:
            a.close(), out.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def markdown(rows, device, args):
    f = lambda s: "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    noise, timed = [r for r in rows if "op" in r], [r for r in rows if "time" in r and not r.get("commit")]
    tagged = [r for r in rows if r.get("commit")]
    out = ["# Hybrid key switching: keys modulo Q P beside the ordinary key switch, noise and time", "",
           "Produced by `python tools/bfv_hybrid_rate.py --reps %d --prof-reps %d` on %s; the method is in the tool's docstring."
           % (args.reps, args.prof_reps, device), "",
           "## Noise", "",
           "`zkfhe_bfv_noise` of the result (the largest of the batch), fresh encryptions in.  P30 = 2^30 - 35; P max is the largest",
           "admissible P coprime to Q (`zkfhe_bfv_hybrid_max_p`).  A pack that does not decrypt to the expected placement is marked.", "",
           "| N | Q bits | w | l | call | n | fresh | ordinary | hybrid P30 | hybrid P max | log2 P max | floor(Q/T)/2 |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in noise:
        cell = lambda k: "%.3g%s" % (r[k], "" if r.get("decrypts", {}).get(k, True) else " (does NOT decrypt)")  # noqa: E731
        out.append("| %d | %d | %d | %d | %s | %d | %d | %s | %s | %s | %.1f | %.3g |" % (
            r["N"], (r["Q"] - 1).bit_length(), r["w"], r["l"], r["op"], r["n"], r["fresh_noise"], cell("ordinary"), cell("hybrid P30"),
            cell("hybrid P max"), math.log2(r["p_max"]), r["half_delta"]))
    out += ["", "## Time", "",
            "The hybrid set (P30) beside the ordinary set at equal (w, l), alternating in one session.  ms, median (lowest - highest).", "",
            "| N | Q bits | w | l | call | n | ordinary wall | hybrid wall | ordinary kernel | hybrid kernel | kernel ratio |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in timed:
        o, h = r["ordinary"], r["hybrid P30"]
        out.append("| %d | %d | %d | %d | %s | %d | %s | %s | %s | %s | %.2f |" % (
            r["N"], (r["Q"] - 1).bit_length(), r["w"], r["l"], r["time"], r["n"], f(o["wall_ms"]), f(h["wall_ms"]), f(o["kernel_ms"]),
            f(h["kernel_ms"]), h["kernel_ms"]["median"] / o["kernel_ms"]["median"]))
    out += ["", "## What the feature is for", "",
            "Per pack size at N = 1024: the widest measured w whose hybrid (P30) noise stays below the ordinary w = 4 noise, with the",
            "kernel time of both.", "",
            "| n | ordinary w = 4 noise | ordinary w = 4 kernel ms | widest w | l | hybrid noise | hybrid kernel ms |", "|---|---|---|---|---|---|---|"]
    for n in (64, 1024):
        base = [r for r in noise if r["N"] == 1024 and r["op"] == "pack" and r["n"] == n and r["w"] == 4]
        wide = [r for r in noise if r["N"] == 1024 and r["op"] == "pack" and r["n"] == n and base and r["hybrid P30"] < base[0]["ordinary"]
                and r["decrypts"]["hybrid P30"]]
        t = {r["w"]: r for r in timed if r["N"] == 1024 and r["time"] == "pack" and r["n"] == n}
        if base and wide and 4 in t:
            best = max(wide, key=lambda r: r["w"])
            if best["w"] in t:
                out.append("| %d | %.3g | %s | %d | %d | %.3g | %s |" % (n, base[0]["ordinary"], f(t[4]["ordinary"]["kernel_ms"]), best["w"], best["l"],
                                                                        best["hybrid P30"], f(t[best["w"]]["hybrid P30"]["kernel_ms"])))
    if tagged:
        out += ["", "## The ordinary rows: parent against this commit", "",
                "`--ordinary-only` runs of the parent commit and of this commit, alternating in one session on the same device: the ordinary",
                "key set alone.  Kernel ms, median (lowest - highest) of each run; the last column says whether this commit's lowest-to-highest",
                "range over its runs overlaps the parent's.", "",
                "| N | w | call | n | parent runs | this commit's runs | ranges overlap |", "|---|---|---|---|---|---|---|"]
        points = list(dict.fromkeys((r["N"], r["w"], r["time"], r["n"]) for r in tagged))
        for pt in points:
            runs = {c: [r["ordinary"]["kernel_ms"] for r in tagged if (r["N"], r["w"], r["time"], r["n"]) == pt and r["commit"] == c]
                    for c in ("parent", "this")}
            if not (runs["parent"] and runs["this"]):
                continue
            lo = {c: min(s["min"] for s in v) for c, v in runs.items()}
            hi = {c: max(s["max"] for s in v) for c, v in runs.items()}
            overlap = lo["this"] <= hi["parent"] and lo["parent"] <= hi["this"]
            out.append("| %d | %d | %s | %d | %s | %s | %s |" % (pt[0], pt[1], pt[2], pt[3], "; ".join(f(s) for s in runs["parent"]),
                                                                "; ".join(f(s) for s in runs["this"]), "yes" if overlap else "NO"))
    if args.asm:
        out += ["", "## Device code of the ordinary instantiations", "",
                "`python tools/device_asm_diff.py <parent> . --pairs 'k_eval_epilogue = k_eval_epilogue<false>' 'k_pack_finish = k_pack_finish<false>'`,",
                "made without a GPU (the new unit and the new kernels exist in this tree only, which the tool counts as differences):", "", "```"]
        out += [l.rstrip() for l in open(args.asm) if not l.startswith(("real", "user", "sys")) and "warning" not in l and l.strip()]
        out += ["```"]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prof-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_hybrid.md"))
    ap.add_argument("--asm", default="", help="the output of tools/device_asm_diff.py, appended as a section")
    ap.add_argument("--ordinary-only", default="", metavar="TAG", help="time the ordinary legs alone; TAG (parent or this) marks the JSON lines")
    ap.add_argument("--package-root", default="", help="the directory of the zk_fhe_amd.py to measure (default: this checkout)")
    ap.add_argument("--from-rows", default="", help="render again from the JSON lines of an earlier run; no GPU")
    ap.add_argument("--device", default="", help="with --from-rows: the device the rows were measured on")
    args = ap.parse_args()
    if args.from_rows:
        rows = [json.loads(line) for line in open(args.from_rows) if line.startswith("{")]
        with open(args.out, "w") as fh:
            fh.write(markdown(rows, args.device, args))
        return
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(2024)
    rows = []
    if args.ordinary_only:
        for prm, w in TIMED:
            keys = key_sets(ctx, zk, np, prm, w, hybrid=False)
            try:
                time_rows(ctx, zk, np, prm, w, keys, args.reps, args.prof_reps, rng, kinds=("ordinary",), tag=args.ordinary_only)
            finally:
                keys[3]["ordinary"].close()
        ctx.close()
        return
    for prm, w in WIDTHS:
        keys = key_sets(ctx, zk, np, prm, w)
        try:
            rows += noise_rows(ctx, zk, np, prm, w, keys, rng)
            if (prm, w) in TIMED:
                rows += time_rows(ctx, zk, np, prm, w, keys, args.reps, args.prof_reps, rng)
        finally:
            for evk in keys[3].values():
                evk.close()
    info = ctx.device_info()
    text = markdown(rows, "%s with %d CUs" % (info["arch"], info["num_cu"]), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
