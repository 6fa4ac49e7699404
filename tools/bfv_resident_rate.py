"""A chain of evaluation calls through host arrays against the same chain on a resident batch (zkfhe_bfv_cts_*), in one process.

The chain: mul_plain by one weight plaintext -> plan_apply with the dense-matrix two-level plan of profiles/bfv_plan.md (all N
diagonals, the default n_baby, 60-bit Q, w = 8) -> the slot sum -> the result on the host.

    host    zkfhe_bfv_mul_plain, zkfhe_bfv_plan_apply, zkfhe_bfv_slot_sum on host arrays, every output array allocated and touched
            once outside the timed region: three uploads and three downloads of the batch, three host range passes
    batch   zkfhe_bfv_cts_store (the checked upload) into a batch made once, zkfhe_bfv_cts_mul_plain, zkfhe_bfv_cts_plan_apply,
            log2(N) x (zkfhe_bfv_cts_apply_galois + zkfhe_bfv_cts_add), zkfhe_bfv_cts_download: one upload and one download

After a warm-up of both the two chains alternate; wall time is around the whole chain, which ends in a call that waits for its result.
Kernel time is the sum of every profiling slot over one chain, from profiled passes of their own (profiling serialises the stream),
the two chains alternating again.  Both are given as the median with the lowest and the highest repeat.  The two results are compared
bit for bit before anything is timed.  With --box the same chain at the k = 13 parameters on the tally of a ballot box of 3 groups:
BallotBox.tally + the host chain against BallotBox.tally_cts + the batch chain.

One JSON line per row (with the launches and the ms of every profiling slot of the last profiled pass), then the markdown table of
profiles/bfv_resident.md.

    python tools/bfv_resident_rate.py [--reps 7] [--prof-reps 3] [--box] [--cts 1,64,1024]

--evk times the chain a third way, alternating with the other two:

    evk     the batch chain with a resident key set (zkfhe_bfv_evk) and the slot sum as one call: zkfhe_bfv_cts_store,
            zkfhe_bfv_cts_mul_plain, zkfhe_bfv_cts_plan_apply, zkfhe_bfv_cts_slot_sum, zkfhe_bfv_cts_download

and prints the tables of profiles/bfv_evk.md: the chain three ways, and the launches per profiling slot of each way.

--key-switch measures the digit-parallel key switch (k_key_switch_digit + k_key_switch_fold, slot 26) against k_key_switch instead of
the chain: zkfhe_bfv_cts_apply_galois (slot 14: the key switch and its epilogue) against zkfhe_bfv_cts_apply_galois_evk (slot 26 plus
slot 14: the same epilogue), and zkfhe_bfv_cts_mul (slot 9) against zkfhe_bfv_cts_mul_evk (slot 26), the two calls alternating, at
1 to 64 ciphertexts, N = 1024 and 4096, a 60-bit Q, w = 8 and 16; the median of --reps repeats with the lowest and the highest.  It
sets ZKFHE_EVK_WIDE_MAX=64 before the library loads, so that the digit-parallel path runs at every count measured.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bfv_bsgs_rate import split  # noqa: E402  (the first K diagonals under the default n_baby)

Q60 = (1 << 60) - 93
SHAPES = [(1024, Q60, 65537, 19), (4096, Q60, 65537, 19)]
CTS = (1, 64, 1024)
W = 8


class Chain:
    """the keys, the plan and the weight of the chain for one parameter set, and the two ways through it"""

    def __init__(self, ctx, zk, np, prm, rng):
        self.ctx, self.zk, self.np, self.prm = ctx, zk, np, prm
        n, q, t = prm[0], prm[1], prm[2]
        sk = ctx.bfv_fhe_keypair(prm, os.urandom(32))[0]
        made = {}

        def key(g):
            if g not in made:
                made[g] = ctx.bfv_galois_keygen(prm, sk, g, base_bits=W)
            return made[g]

        def plain(shape):
            x = rng.integers(-(t // 2), t // 2 + 1, size=shape + (n,))
            return np.where(x < 0, x + q, x).astype(np.uint64)

        baby, giant = split(n, n)   # the dense matrix
        gb, gg = ([zk.bfv_galois_element(prm, *e) for e in lst] for lst in (baby, giant))
        bk, hk = ([key(g) for g in lst] for lst in (gb, gg))
        stack = lambda ks, i: np.array([k[i] for k in ks])  # noqa: E731
        self.plan = ctx.bfv_plan_bsgs(prm, gb, stack(bk, 0), stack(bk, 1), gg, stack(hk, 0), stack(hk, 1), plain((len(gg), len(gb))), base_bits=W)
        self.weight = plain(())
        self.elements = [int(g) for g in zk.bfv_slot_sum_elements(prm)]
        self.sum_keys = [key(g) for g in self.elements]
        self.sk0, self.sk1 = stack(self.sum_keys, 0), stack(self.sum_keys, 1)

    def buffers(self, count):
        """what a caller keeps between chains: three pairs of host arrays (touched), two batches"""
        np, n = self.np, self.prm[0]
        host = [[np.zeros((count, n), dtype=np.uint64) for _ in range(2)] for _ in range(3)]
        return host, self.ctx.bfv_cts_zeros(self.prm, count), self.ctx.bfv_cts_zeros(self.prm, count)

    def host(self, c0, c1, bufs):
        ctx, prm, count = self.ctx, self.prm, c0.shape[0]
        ctx._call("zkfhe_bfv_mul_plain", prm, count, c0, c1, 1, self.weight, *bufs[0])
        ctx._call("zkfhe_bfv_plan_apply", self.plan._handle(), count, *bufs[0], *bufs[1])
        ctx._call("zkfhe_bfv_slot_sum", prm, count, *bufs[1], self.sk0, self.sk1, W, *bufs[2])
        return bufs[2]

    def on_batch(self, x, rot, out):
        """the chain on what x holds, into the host arrays out"""
        x.mul_plain(self.weight, out=x)
        self.plan.apply_cts(self.ctx, x, out=x)
        for g, (k0, k1) in zip(self.elements, self.sum_keys):
            x.apply_galois(g, k0, k1, base_bits=W, out=rot)
            x.add(rot, out=x)
        self.ctx._call("zkfhe_bfv_cts_download", x._handle(), 0, x.n, *out)
        return out

    def batch(self, c0, c1, x, rot, out):
        x.store(c0, c1)
        return self.on_batch(x, rot, out)

    def make_evk(self):
        self.evk = self.ctx.bfv_evk(self.prm, W, None, self.elements, self.sk0, self.sk1)

    def on_batch_evk(self, x, out):
        """the chain on what x holds with the resident keys, the slot sum one call, into the host arrays out"""
        x.mul_plain(self.weight, out=x)
        self.plan.apply_cts(self.ctx, x, out=x)
        x.slot_sum(self.evk, out=x)
        self.ctx._call("zkfhe_bfv_cts_download", x._handle(), 0, x.n, *out)
        return out

    def batch_evk(self, c0, c1, x, out):
        x.store(c0, c1)
        return self.on_batch_evk(x, out)

    def close(self):
        self.plan.close()
        if getattr(self, "evk", None):
            self.evk.close()


def kernel_ms(ctx, zk, fn):
    ctx.prof_enable(True)   # resets the slots
    fn()
    prof = {s: ctx.prof_read(s) for s in range(zk.PROF_BFV_KEY_SWITCH_WIDE + 1)}
    ctx.prof_enable(False)
    return sum(p["total_ms"] for p in prof.values()), {s: [p["launches"], round(p["total_ms"], 4)] for s, p in prof.items() if p["launches"]}


def compare(ctx, zk, np, legs, reps, prof_reps):
    """legs: {"host": fn, "batch": fn}, each returning its two result arrays -> wall and kernel ms per leg (lists), and the slots of
    the last profiled pass"""
    res = {name: [a.copy() for a in fn()] for name, fn in legs.items()}   # warm-up: tables, arena, code objects
    assert all(np.array_equal(a, b) for name in res for a, b in zip(res["host"], res[name])), "the chains differ"
    wall, kern, slots = {name: [] for name in legs}, {name: [] for name in legs}, {}
    for _ in range(reps):
        for name, fn in legs.items():   # A/B
            t0 = time.perf_counter()
            fn()   # ends in a call that waits for its result
            wall[name].append((time.perf_counter() - t0) * 1e3)
    for _ in range(prof_reps):
        for name, fn in legs.items():
            ms, slots[name] = kernel_ms(ctx, zk, fn)
            kern[name].append(ms)
    return wall, kern, slots


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def row_of(what, prm, count, wall, kern, slots):
    """slots: per profiling slot [launches, ms] of the last profiled pass"""
    row = {"what": what, "N": prm[0], "Q": prm[1], "T": prm[2], "w": W, "cts": count}
    for name in wall:
        row[name] = {"wall_ms": stats(wall[name]), "kernel_ms": stats(kern[name]), "slots": slots[name]}
    row["wall_ratio"] = round(row["host"]["wall_ms"]["median"] / row["batch"]["wall_ms"]["median"], 2)
    row["kernel_ratio"] = round(row["host"]["kernel_ms"]["median"] / row["batch"]["kernel_ms"]["median"], 3)
    if "evk" in row:
        row["evk_wall_ratio"] = round(row["host"]["wall_ms"]["median"] / row["evk"]["wall_ms"]["median"], 2)
    print(json.dumps(row), flush=True)
    return row


def measure(a):
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    rows = []
    for prm in SHAPES:
        n, q = prm[0], prm[1]
        chain = Chain(ctx, zk, np, prm, rng)
        if a.evk:
            chain.make_evk()
        for count in a.cts:
            c0 = rng.integers(0, q, size=(count, n), dtype=np.uint64)   # the cost does not depend on the values
            c1 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
            host, x, rot = chain.buffers(count)
            out = [np.zeros((count, n), dtype=np.uint64) for _ in range(2)]
            legs = {"host": lambda: chain.host(c0, c1, host), "batch": lambda: chain.batch(c0, c1, x, rot, out)}
            if a.evk:
                out3 = [np.zeros((count, n), dtype=np.uint64) for _ in range(2)]
                legs["evk"] = lambda: chain.batch_evk(c0, c1, x, out3)
            rows.append(row_of("chain", prm, count, *compare(ctx, zk, np, legs, a.reps, a.prof_reps)))
            x.close(), rot.close()
        chain.close()
    if a.box:
        rows.append(box_row(ctx, zk, np, rng, a))
    ctx.close()
    return rows


def box_row(ctx, zk, np, rng, a):
    """3 groups of 2 k = 13 proofs each; tally + chain from the box through the host and on the device"""
    from zk_fhe_amd import inputs
    from oracle import circuit_ref as C
    os.environ.setdefault("ZKFHE_TABLE_GB", "4")
    cfgj = json.load(open(os.path.join(ROOT, "tests", "golden", "bfv", "bfv_config.json")))
    p = C.BfvParams()
    n, prm = 1024, (1024, p.Q, p.T, p.B)
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(n)), prm, zk.BfvConfig.from_pinning(cfgj), replay=True)
    vk = pk.export_vk()
    items = []
    for j in range(6):
        proof, inst, _ = pk.prove(json.dumps(inputs.generate(n, p.Q, p.T, p.B, seed=7000 + j, key_seed=0)), b"resident-%d" % j)
        items.append((inst, proof))
    pk.destroy()
    srs.destroy()
    pk0, pk1, _, _ = zk.bfv_instance_words(prm, items[0][0])
    chain = Chain(ctx, zk, np, prm, rng)
    if a.evk:
        chain.make_evk()
    box = zk.BallotBox(ctx, vk, prm, pk0, pk1, n_groups=3)
    assert all(s == zk.BALLOT_COUNTED for s, _ in box.add(items, [0, 1, 2, 0, 1, 2]))
    host, x, rot = chain.buffers(3)
    out = [np.zeros((3, n), dtype=np.uint64) for _ in range(2)]

    def through_host():
        c0, c1, _ = box.tally()
        return chain.host(c0, c1, host)

    def on_device():
        box.tally_cts(out=x)
        return chain.on_batch(x, rot, out)

    legs = {"host": through_host, "batch": on_device}
    if a.evk:
        out3 = [np.zeros((3, n), dtype=np.uint64) for _ in range(2)]

        def on_device_evk():
            box.tally_cts(out=x)
            return chain.on_batch_evk(x, out3)

        legs["evk"] = on_device_evk
    row = row_of("box_tally_chain", prm, 3, *compare(ctx, zk, np, legs, a.reps, a.prof_reps))
    x.close(), rot.close(), box.close(), chain.close()
    return row


KS_COUNTS = (1, 2, 3, 4, 8, 16, 32, 64)


def key_switch_rows(a):
    """the key-switch kernels of one call, sequential against digit-parallel, from the profiling slots"""
    os.environ.setdefault("ZKFHE_EVK_WIDE_MAX", str(max(KS_COUNTS)))   # before the library loads: the bound itself is what is measured
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    rng = np.random.default_rng(1)
    GAL, REL, EPI, WIDE = zk.PROF_BFV_GALOIS, zk.PROF_BFV_RELIN, zk.PROF_BFV_EVAL_EPILOGUE, zk.PROF_BFV_KEY_SWITCH_WIDE
    rows = []

    def slots_ms(fn, slots):
        ctx.prof_enable(True)
        fn()
        ms = sum(ctx.prof_read(s)["total_ms"] for s in slots)
        ctx.prof_enable(False)
        return ms

    for prm in SHAPES:
        n, q = prm[0], prm[1]
        for w in (8, 16):
            sk = ctx.bfv_fhe_keypair(prm, os.urandom(32))[0]
            gk0, gk1 = ctx.bfv_galois_keygen(prm, sk, 5, base_bits=w)
            rlk = ctx.bfv_relin_keygen(prm, sk, base_bits=w)
            evk = ctx.bfv_evk(prm, w, rlk, [5], gk0[None], gk1[None])
            l = zk.bfv_relin_digits(prm, w)
            for count in KS_COUNTS:
                assert count <= ctx.bfv_evk_wide_max(prm, w), "the digit-parallel path is not forced"
                c = [rng.integers(0, q, size=(count, n), dtype=np.uint64) for _ in range(4)]
                x, y, out = ctx.bfv_cts(prm, c[0], c[1]), ctx.bfv_cts(prm, c[2], c[3]), ctx.bfv_cts_zeros(prm, count)
                for kind, old, new, old_slots, new_slots in [
                        ("galois", lambda: x.apply_galois(5, gk0, gk1, base_bits=w, out=out), lambda: x.apply_galois_evk(5, evk, out=out), (GAL,), (WIDE, GAL)),
                        ("relin", lambda: x.mul(y, rlk[0], rlk[1], base_bits=w, out=out), lambda: x.mul_evk(y, evk, out=out), (REL,), (WIDE,))]:
                    old(), new()   # warm-up
                    ms = {"seq": [], "wide": []}
                    for _ in range(a.reps):
                        ms["seq"].append(slots_ms(old, old_slots))
                        ms["wide"].append(slots_ms(new, new_slots))
                    row = {"what": "key_switch", "kind": kind, "N": n, "w": w, "l": l, "cts": count, "grid_seq": 5 * count, "grid_wide": 5 * count * l,
                           "num_cu": ctx.device_info()["num_cu"], "seq_ms": stats(ms["seq"]), "wide_ms": stats(ms["wide"])}
                    row["wide_below_seq"] = row["wide_ms"]["max"] < row["seq_ms"]["min"]
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                x.close(), y.close(), out.close()
            evk.close()
    ctx.close()
    rng_of = lambda s: "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    print("\n| key switch | N | w | l | ciphertexts | grid k_key_switch | grid k_key_switch_digit | ms k_key_switch: median (min .. max) of %d | "
          "ms digit-parallel | highest digit-parallel < lowest k_key_switch |\n|---|---|---|---|---|---|---|---|---|---|" % a.reps)
    for r in rows:
        print("| %s | %d | %d | %d | %d | %d | %d | %s | %s | %s |" % (r["kind"], r["N"], r["w"], r["l"], r["cts"], r["grid_seq"], r["grid_wide"],
                                                                      rng_of(r["seq_ms"]), rng_of(r["wide_ms"]), "yes" if r["wide_below_seq"] else "no"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prof-reps", type=int, default=3)
    ap.add_argument("--box", action="store_true", help="also the chain on the tally of a ballot box of 3 groups (makes six k = 13 proofs)")
    ap.add_argument("--evk", action="store_true", help="also the batch chain with a resident key set and the slot sum as one call")
    ap.add_argument("--key-switch", action="store_true", help="the digit-parallel key switch against k_key_switch instead of the chain")
    ap.add_argument("--cts", type=lambda v: tuple(int(x) for x in v.split(",")), default=CTS, help="the ciphertext counts of the chain rows")
    a = ap.parse_args()
    if a.key_switch:
        return key_switch_rows(a)
    rows = measure(a)
    rng_of = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    print("\n| chain | N | Q bits | ciphertexts | wall ms host arrays: median (min .. max) of %d | wall ms batch | host / batch | kernel ms host arrays: median (min .. max) of %d | "
          "kernel ms batch | host / batch |\n|---|---|---|---|---|---|---|---|---|---|" % (a.reps, a.prof_reps))
    for r in rows:
        print("| %s | %d | %d | %d | %s | %s | %.2f | %s | %s | %.3f |" % (
            r["what"], r["N"], r["Q"].bit_length(), r["cts"], rng_of(r["host"]["wall_ms"]), rng_of(r["batch"]["wall_ms"]), r["wall_ratio"],
            rng_of(r["host"]["kernel_ms"]), rng_of(r["batch"]["kernel_ms"]), r["kernel_ratio"]))

    if a.evk:
        print("\n| chain | N | ciphertexts | wall ms host arrays | wall ms batch | wall ms batch + key set | host / key set | kernel ms host arrays | "
              "kernel ms batch | kernel ms batch + key set |\n|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %d | %d | %s | %s | %s | %.2f | %s | %s | %s |" % (
                r["what"], r["N"], r["cts"], rng_of(r["host"]["wall_ms"]), rng_of(r["batch"]["wall_ms"]), rng_of(r["evk"]["wall_ms"]), r["evk_wall_ratio"],
                rng_of(r["host"]["kernel_ms"]), rng_of(r["batch"]["kernel_ms"]), rng_of(r["evk"]["kernel_ms"])))
        print("\n| chain | N | ciphertexts | slot | host arrays: launches, ms | batch: launches, ms | batch + key set: launches, ms |\n|---|---|---|---|---|---|---|")
        for r in rows:
            if r["cts"] > 3:
                continue
            used = sorted({int(s) for name in ("host", "batch", "evk") for s in r[name]["slots"]})
            cell = lambda name, s: "%d, %.3f" % tuple(r[name]["slots"][s]) if s in r[name]["slots"] else "none"  # noqa: E731
            for s in used:
                print("| %s | %d | %d | %d | %s | %s | %s |" % (r["what"], r["N"], r["cts"], s, cell("host", s), cell("batch", s), cell("evk", s)))


if __name__ == "__main__":
    main()
