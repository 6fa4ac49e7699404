"""Ring packing (zkfhe_bfv_cts_pack) against its composition by hand from the batch calls, and the noise of a packed result.

    fused     zkfhe_bfv_cts_pack with a resident key set: one prepare launch, then per level the key switch that reads its digits
              from the two operands and k_pack_finish
    by hand   the definition from the existing calls on batches, level by level: zkfhe_bfv_cts_mul_monomial by x^(2N - pos), then per
              pack level two zkfhe_bfv_cts_select, zkfhe_bfv_cts_mul_monomial, zkfhe_bfv_cts_add twice, zkfhe_bfv_cts_apply_galois_evk,
              zkfhe_bfv_cts_add, and per trace level zkfhe_bfv_cts_apply_galois_evk and zkfhe_bfv_cts_add.  Every batch it needs is
              made before the clock starts.  It leaves out the scaling by N^-1 and the zero padding, for which there is no call on
              batches (n is a power of two at every point): that favours it, and its bits are not those of the fused call
              (tests/test_gpu_bfv_pack.py compares the bits, with the scaling done on the host).

Time: after a warm-up of both the two alternate; wall time is around the whole call or chain, which ends in a call that waits for its
result; kernel time is the sum of every profiling slot, from profiled passes of their own (profiling serialises the stream).  Both
are the median with the lowest and the highest repeat.
Noise: n fresh encryptions of random plaintexts are packed at random positions; the result must decrypt to the expected placement,
and zkfhe_bfv_noise of it stands beside floor(Q/T)/2 and the header's sufficient bound max_i noise(a_i) + (N - 1) l N (2^w - 1) B.

One JSON line per point, then the markdown of profiles/bfv_pack.md, written to --out.

    python tools/bfv_pack_rate.py [--reps 5] [--prof-reps 3] [--out profiles/bfv_pack.md] [--parent-bench LINE]... [--bench LINE]...

--parent-bench and --bench take result lines of `python bench.py --gpus 1` (each may be given more than once, in the order run); the
regression section quotes their metric, value, ms per step, steps and the digest of the last timed proof.  --from-rows FILE renders
the markdown again from the JSON lines of an earlier run (its device and repeat counts are given with --device, --reps, --prof-reps)
and needs no GPU.
"""
import argparse
import json
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
POINTS = [(K13, 4, 1), (K13, 4, 64), (K13, 4, 1024), (K13, 8, 1), (K13, 8, 64), (K13, 8, 1024), (P4096, 8, 4096), (P4096, 16, 4096)]


def pack_elements(n_ring):
    return [(1 << l) + 1 for l in range(1, n_ring.bit_length())]


class Hand:
    """the batches of the composition by hand for n inputs (a power of two), made once"""

    def __init__(self, ctx, np, prm, n, evk):
        self.ctx, self.np, self.prm, self.n, self.evk = ctx, np, prm, n, evk
        self.levels = []
        h = n
        while h > 1:
            h //= 2
            self.levels.append([ctx.bfv_cts_zeros(prm, h) for _ in range(5)])   # e, o, total, diff, next
        self.first = ctx.bfv_cts_zeros(prm, n)
        self.rot = ctx.bfv_cts_zeros(prm, 1)

    def run(self, a, shift):
        n_ring = self.prm[0]
        cur = a.mul_monomial(shift, out=self.first)
        lv = 0
        for lv, (e, o, total, diff, nxt) in enumerate(self.levels, 1):
            h = e.n
            cur.select(range(h), out=e)
            cur.select(range(h, 2 * h), out=o)
            o.mul_monomial(n_ring >> lv, out=o)
            e.add(o, out=total)
            e.sub(o, out=diff)
            diff.apply_galois_evk((1 << lv) + 1, self.evk, out=diff)
            cur = total.add(diff, out=nxt)
        for lv in range(lv + 1, n_ring.bit_length()):
            cur.apply_galois_evk((1 << lv) + 1, self.evk, out=self.rot)
            cur.add(self.rot, out=cur)
        return cur

    def close(self):
        for b in [x for lvl in self.levels for x in lvl] + [self.first, self.rot]:
            b.close()


def kernel_ms(ctx, zk, fn):
    ctx.prof_enable(True)   # resets the slots
    fn()
    prof = {s: ctx.prof_read(s) for s in range(zk.PROF_BFV_PACK + 1)}
    ctx.prof_enable(False)
    return sum(p["total_ms"] for p in prof.values()), sum(p["launches"] for p in prof.values())


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def measure(ctx, zk, np, prm, w, n, keys, reps, prof_reps, rng):
    n_ring, q, t, b = prm
    sk, pk0, pk1, gk0, gk1, evk = keys
    m = rng.integers(-(t // 2), t // 2 + 1, size=(n, n_ring))
    m = np.where(m < 0, m + q, m).astype(np.uint64)
    ct = ctx.bfv_encrypt(prm, pk0, pk1, m, os.urandom(32))
    pos = rng.integers(0, n_ring, size=n, dtype=np.uint64)
    shift = (2 * n_ring - pos) % np.uint64(2 * n_ring)
    fresh = int(ctx.bfv_noise(prm, sk, ct["c0"], ct["c1"]).max())
    l = zk.bfv_relin_digits(prm, w)
    row = {"N": n_ring, "Q": q, "T": t, "w": w, "l": l, "n": n, "half_delta": (q // t) // 2, "fresh_noise": fresh,
           "bound": fresh + (n_ring - 1) * l * n_ring * ((1 << w) - 1) * b}
    a, out = ctx.bfv_cts(prm, ct["c0"], ct["c1"]), ctx.bfv_cts_zeros(prm, 1)
    hand = Hand(ctx, np, prm, n, evk)
    legs = {"fused": lambda: a.pack(n, evk, pos=pos, out=out), "by_hand": lambda: hand.run(a, shift)}
    try:
        for fn in legs.values():
            fn()   # warm-up: tables, arena, code objects
        o0, o1 = out.download()
        want = np.zeros(n_ring, dtype=np.uint64)
        want[n_ring - 1 - np.arange(n) * (n_ring // n)] = m[np.arange(n), n_ring - 1 - pos.astype(np.int64)]
        row["decrypts"] = bool(np.array_equal(ctx.bfv_decrypt(prm, sk, o0, o1)[0], want))
        row["noise"] = int(ctx.bfv_noise(prm, sk, o0, o1)[0])   # against the nearest plaintext: meaningful where decrypts is true
        wall, kern, launches = {k: [] for k in legs}, {k: [] for k in legs}, {}
        for _ in range(reps):
            for name, fn in legs.items():   # A/B
                t0 = time.perf_counter()
                fn()   # waits for its result
                wall[name].append((time.perf_counter() - t0) * 1e3)
        for _ in range(prof_reps):
            for name, fn in legs.items():
                ms, launches[name] = kernel_ms(ctx, zk, fn)
                kern[name].append(ms)
        for name in legs:
            row[name] = {"wall_ms": stats(wall[name]), "kernel_ms": stats(kern[name]), "launches": launches[name]}
    finally:
        hand.close()
        for x in (a, out):
            x.close()
    print(json.dumps(row), flush=True)
    return row


def markdown(rows, device, args):
    f = lambda s: "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    out = ["# Ring packing: the fused call against the composition by hand, and the noise of a packed result", "",
           "Produced by `python tools/bfv_pack_rate.py --reps %d --prof-reps %d` on %s; the method is in the tool's docstring."
           % (args.reps, args.prof_reps, device), "",
           "## Time", "",
           "`zkfhe_bfv_cts_pack` with a resident key set against the by-hand composition of the batch calls (which leaves out the scaling",
           "by N^-1: that favours it).  ms, median (lowest - highest); launches are those of one call or chain.", "",
           "| N | Q bits | w | l | n | fused wall | by hand wall | fused kernel | by hand kernel | fused launches | by hand launches |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %d | %d | %d | %d | %s | %s | %s | %s | %d | %d |" % (
            r["N"], (r["Q"] - 1).bit_length(), r["w"], r["l"], r["n"], f(r["fused"]["wall_ms"]), f(r["by_hand"]["wall_ms"]),
            f(r["fused"]["kernel_ms"]), f(r["by_hand"]["kernel_ms"]), r["fused"]["launches"], r["by_hand"]["launches"]))
    out += ["", "## Noise", "",
            "n fresh encryptions packed at random positions.  `noise` is `zkfhe_bfv_noise` of the result (against the nearest plaintext, so it",
            "means what it says only where the result decrypts to the expected placement); `bound` is the header's sufficient bound.", "",
            "| N | Q bits | T | w | n | fresh noise | noise of the pack | floor(Q/T)/2 | bound | decrypts |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %d | %d | %d | %d | %d | %.3g | %.3g | %.3g | %s |" % (
            r["N"], (r["Q"] - 1).bit_length(), r["T"], r["w"], r["n"], r["fresh_noise"], r["noise"], r["half_delta"], r["bound"],
            "yes" if r["decrypts"] else "NO"))
    if args.parent_bench or args.bench:
        out += ["", "## Regression", "",
                "`python bench.py --gpus 1` of the parent commit and of this commit, alternating in one session on the same device.  The",
                "prover is not touched, so a difference is the spread of the box.", "",
                "| commit | metric | value | ms per step | steps | sha256 of the last timed proof |", "|---|---|---|---|---|---|"]
        for name, lines in (("parent", args.parent_bench), ("this commit", args.bench)):
            for line in lines:
                r = json.loads(line)
                out.append("| %s | %s | %.1f %s | %.3f | %d | `%s` |" % (name, r["metric"], r["value"], r["unit"], r["ms_per_step"], r["steps"],
                                                                      r["config"]["last_timed_proof"]["sha256"][:16]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prof-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfv_pack.md"))
    ap.add_argument("--parent-bench", action="append", default=[], help="a bench.py result line of the parent commit (repeatable)")
    ap.add_argument("--bench", action="append", default=[], help="a bench.py result line of this commit (repeatable)")
    ap.add_argument("--from-rows", default="", help="render again from the JSON lines of an earlier run; no GPU")
    ap.add_argument("--device", default="", help="with --from-rows: the device the rows were measured on")
    ap.add_argument("--points", default="", help="N:w:n,... instead of the default points")
    args = ap.parse_args()
    if args.from_rows:
        rows = [json.loads(line) for line in open(args.from_rows) if line.startswith('{"N"')]
        with open(args.out, "w") as fh:
            fh.write(markdown(rows, args.device, args))
        return
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(2021)
    points = POINTS
    if args.points:
        by_n = {K13[0]: K13, P4096[0]: P4096}
        points = [(by_n[int(a)], int(b), int(c)) for a, b, c in (p.split(":") for p in args.points.split(","))]
    rows, made = [], {}
    for prm, w, n in points:
        if (prm, w) not in made:
            sk, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
            ks = [ctx.bfv_galois_keygen(prm, sk, g, base_bits=w) for g in pack_elements(prm[0])]
            gk0, gk1 = np.array([k[0] for k in ks]), np.array([k[1] for k in ks])
            made[(prm, w)] = (sk, pk0, pk1, gk0, gk1, ctx.bfv_evk(prm, w, None, pack_elements(prm[0]), gk0, gk1))
        rows.append(measure(ctx, zk, np, prm, w, n, made[(prm, w)], args.reps, args.prof_reps, rng))
    for k in made.values():
        k[5].close()
    info = ctx.device_info()
    text = markdown(rows, "%s with %d CUs" % (info["arch"], info["num_cu"]), args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    ctx.close()


if __name__ == "__main__":
    main()
