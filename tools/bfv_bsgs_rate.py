"""The baby-step/giant-step linear transform against the flat one: zkfhe_bfv_linear_transform_bsgs and zkfhe_bfv_linear_transform on
the same K diagonals in the same process.  The three parts of profiles/bfv_bsgs.md:

  --static    registers, LDS and scratch of the kernels of bfv_linear.hip from the compiler's resource report (no GPU)
  --counts    keys, key bytes, transforms and pointwise products per call, counted (no GPU)
  (default)   measured on the GPU: after a warm-up the two calls and zkfhe_bfv_plan_apply of a plan of each (made outside the timed
              region) alternate A/B/C/D, wall time around each call, then one profiled pass of each for the kernel times of the
              zkfhe_prof_* slots.  One JSON line per row, then the tables: the two calls as in profiles/bfv_bsgs.md, and the plans
              beside them with their creation time and device bytes (profiles/bfv_plan.md).

K diagonals are the first K of the order of zk.bfv_matrix_diagonals (unswapped offsets 0 .. N/2 - 1, then the swapped ones); the BSGS
side splits them as zk.bfv_matrix_bsgs does with its default n_baby.  Diagonals and ciphertexts are random: no cost depends on a
value.  The flat side's K keys are made once, outside the timed region.

    python tools/bfv_bsgs_rate.py [--reps 3] > bsgs.txt
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q60 = (1 << 60) - 93
SHAPES = [(1024, 12289, (16, 64, 256, 1024)), (4096, 65537, (64, 512))]   # N, T, the K
CTS = (1, 16)
W = 8
NAMES = {6: "rns_ntt", 10: "epilogue", 16: "hoist", 17: "accumulate", 18: "inner", 19: "giant"}


def split(n, K):
    """(baby (steps, swap), giant (steps, swap)) of the first K diagonals under the default n_baby"""
    half = n // 2
    nb = 1 << -(-(n.bit_length() - 1) // 2)
    giants = [(i * nb, sw) for sw in (False, True) for i in range(-(-min(max(K - sw * half, 0), half) // nb))]
    return [(b, False) for b in range(min(nb, K))], giants


def relin_digits(q, w):
    return -(-(q - 1).bit_length() // w)


def counts():
    lines = ["| N | K | keys flat | keys BSGS | key MB flat | key MB BSGS | forward transforms per call flat (keys + diagonals + per ciphertext) | "
             "BSGS | inverse per ciphertext flat | BSGS | products per (index, prime, ciphertext) flat | BSGS |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, t, ks in SHAPES:
        l = relin_digits(Q60, W)
        for K in ks:
            baby, giant = split(n, K)
            nb, ng = len(baby), len(giant)
            kb, kg = sum(b != (0, False) for b in baby), sum(g != (0, False) for g in giant)
            kf = K - 1   # offset 0 is g = 1
            mb = lambda keys: keys * 2 * l * n * 8 / 1e6  # noqa: E731
            lines.append("| %d | %d | %d | %d | %.1f | %.1f | %d + %d + %d | %d + %d + %d | 2 | %d | %d | %d |" % (
                n, K, kf, kb + kg, mb(kf), mb(kb + kg), 2 * l * kf, K, l + 1, 2 * l * (kb + kg), nb * ng, (l + 1) * (1 + ng), 2 + 2 * ng,
                2 * kf * l + 2 * K, 2 * kb * l + 2 * nb * ng + 2 * kg * l))
    return "\n".join(lines) + "\n"


def static():
    sys.path.insert(0, os.path.join(ROOT, "zk-fhe_amd"))
    import build
    cmd = [build.hipcc()] + build.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                          os.path.join(build.CSRC, "bfv_linear.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], stdout=subprocess.PIPE, text=True).stdout.strip()
            cur = {"kernel": re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))}
            rows.append(cur)
        else:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    lines = ["| kernel | VGPRs | SGPRs | static LDS bytes | scratch bytes/lane | waves/SIMD |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| `%s` | %s | %s | %s | %s | %s |" % (r["kernel"], r["VGPRs"], r["TotalSGPRs"], r["LDS"], r["ScratchSize"], r["Occupancy"]))
    return "\n".join(lines) + "\n"


def measure(reps):
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    rows = []
    for n, t, ks in SHAPES:
        prm, half, q = (n, Q60, t, 19), n // 2, Q60
        sk = ctx.bfv_fhe_keypair(prm, os.urandom(32))[0]
        order = [(k, sw) for sw in (False, True) for k in range(half)][:max(ks)]
        made = {}

        def keys(elems):
            for e in elems:
                if e not in made:
                    made[e] = ctx.bfv_galois_keygen(prm, sk, zk.bfv_galois_element(prm, *e), base_bits=W)
            return np.array([made[e][0] for e in elems]), np.array([made[e][1] for e in elems])

        def plain(shape):
            x = rng.integers(-(t // 2), t // 2 + 1, size=shape + (n,))
            return np.where(x < 0, x + q, x).astype(np.uint64)

        for K in ks:
            flat = order[:K]
            baby, giant = split(n, K)
            gf, gb, gg = ([zk.bfv_galois_element(prm, *e) for e in lst] for lst in (flat, baby, giant))
            fk0, fk1 = keys(flat)
            bk0, bk1 = keys(baby)
            hk0, hk1 = keys(giant)
            fd, bd = plain((K,)), plain((len(giant), len(baby)))
            plans, create_ms = {}, {}
            for name, make in (("flat", lambda: ctx.bfv_plan(prm, gf, fk0, fk1, fd, base_bits=W)),
                               ("bsgs", lambda: ctx.bfv_plan_bsgs(prm, gb, bk0, bk1, gg, hk0, hk1, bd, base_bits=W))):
                make().close()   # warm-up: tables, arena
                t0 = time.perf_counter()
                plans[name] = make()   # waits for its device work
                create_ms[name] = (time.perf_counter() - t0) * 1e3
            for count in CTS:
                c0 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
                c1 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
                calls = {"flat": lambda: ctx.bfv_linear_transform(prm, c0, c1, gf, fk0, fk1, fd, base_bits=W),
                         "bsgs": lambda: ctx.bfv_linear_transform_bsgs(prm, c0, c1, gb, bk0, bk1, gg, hk0, hk1, bd, base_bits=W),
                         "flat_plan": lambda: plans["flat"].apply(c0, c1),
                         "bsgs_plan": lambda: plans["bsgs"].apply(c0, c1)}
                for fn in calls.values():
                    fn()   # warm-up: tables, arena
                wall = {name: [] for name in calls}
                for _ in range(reps):
                    for name, fn in calls.items():   # A/B/C/D
                        t0 = time.perf_counter()
                        fn()   # waits for its result
                        wall[name].append((time.perf_counter() - t0) * 1e3)
                row = dict(N=n, T=t, w=W, K=K, cts=count, n_baby=len(baby), n_giant=len(giant))
                for name, fn in calls.items():
                    ctx.prof_enable(True)
                    fn()
                    prof = {s: ctx.prof_read(s) for s in range(5, 20)}
                    ctx.prof_enable(False)
                    row[name] = dict(wall_ms=[round(x, 3) for x in wall[name]],
                                     kernel_ms={NAMES.get(s, str(s)): round(p["total_ms"], 4) for s, p in prof.items() if p["launches"]})
                row["ratio"] = round(min(wall["flat"]) / min(wall["bsgs"]), 2)
                for name, plan in plans.items():
                    row[name + "_plan"].update(create_ms=round(create_ms[name], 3), device_bytes=plan.info()["device_bytes"])
                print(json.dumps(row), flush=True)
                rows.append(row)
            for plan in plans.values():
                plan.close()
    ctx.close()
    lines = ["| N | K | n_baby x n_giant | ciphertexts | wall ms flat (min of %d) | wall ms BSGS | flat / BSGS | kernel ms flat | kernel ms BSGS | BSGS inner ms | BSGS giant ms |" % reps,
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        kf, kb = r["flat"]["kernel_ms"], r["bsgs"]["kernel_ms"]
        lines.append("| %d | %d | %d x %d | %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.4f | %.4f |" % (
            r["N"], r["K"], r["n_baby"], r["n_giant"], r["cts"], min(r["flat"]["wall_ms"]), min(r["bsgs"]["wall_ms"]), r["ratio"],
            sum(kf.values()), sum(kb.values()), kb.get("inner", 0.0), kb.get("giant", 0.0)))
    for n, _, ks in SHAPES:
        for count in CTS:
            wins = [r["K"] for r in rows if r["N"] == n and r["cts"] == count and r["ratio"] > 1.0]
            lines.append("N = %d, %d ciphertext(s): the smallest K at which BSGS wins on wall time: %s" % (n, count, min(wins) if wins else "none of %s" % (ks,)))
    lines += ["", "| N | K | ciphertexts | wall ms flat (min of %d) | flat plan apply | flat / plan | wall ms BSGS | BSGS plan apply | BSGS / plan | "
              "kernel ms flat plan | kernel ms BSGS plan | create ms flat plan | BSGS plan | plan MB flat | BSGS |" % reps,
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        w = {name: min(r[name]["wall_ms"]) for name in ("flat", "flat_plan", "bsgs", "bsgs_plan")}
        lines.append("| %d | %d | %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %.3f | %.3f | %.1f | %.1f | %.1f | %.1f |" % (
            r["N"], r["K"], r["cts"], w["flat"], w["flat_plan"], w["flat"] / w["flat_plan"], w["bsgs"], w["bsgs_plan"], w["bsgs"] / w["bsgs_plan"],
            sum(r["flat_plan"]["kernel_ms"].values()), sum(r["bsgs_plan"]["kernel_ms"].values()), r["flat_plan"]["create_ms"],
            r["bsgs_plan"]["create_ms"], r["flat_plan"]["device_bytes"] / 1e6, r["bsgs_plan"]["device_bytes"] / 1e6))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.static:
        sys.stdout.write(static())
    elif a.counts:
        sys.stdout.write(counts())
    else:
        measure(a.reps)


if __name__ == "__main__":
    main()
