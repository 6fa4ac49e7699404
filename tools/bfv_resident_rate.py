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

    python tools/bfv_resident_rate.py [--reps 7] [--prof-reps 3] [--box]
"""
import argparse
import ctypes
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
        self.u64p = ctypes.POINTER(ctypes.c_uint64)

    def buffers(self, count):
        """what a caller keeps between chains: three pairs of host arrays (touched), two batches"""
        np, n = self.np, self.prm[0]
        host = [[np.zeros((count, n), dtype=np.uint64) for _ in range(2)] for _ in range(3)]
        return host, self.ctx.bfv_cts_zeros(self.prm, count), self.ctx.bfv_cts_zeros(self.prm, count)

    def host(self, c0, c1, bufs):
        ctx, prm, count = self.ctx, self.prm, c0.shape[0]
        ctx._bfv("zkfhe_bfv_mul_plain", "nppnppp", prm, count, c0, c1, 1, self.weight, *bufs[0])
        f = ctx.lib.zkfhe_bfv_plan_apply
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [self.u64p] * 4
        ctx._check(f(ctx.h, self.plan._handle(), count, *[a.ctypes.data_as(self.u64p) for a in (*bufs[0], *bufs[1])]))
        ctx._bfv("zkfhe_bfv_slot_sum", "nppppipp", prm, count, *bufs[1], self.sk0, self.sk1, W, *bufs[2])
        return bufs[2]

    def on_batch(self, x, rot, out):
        """the chain on what x holds, into the host arrays out"""
        x.mul_plain(self.weight, out=x)
        self.plan.apply_cts(self.ctx, x, out=x)
        for g, (k0, k1) in zip(self.elements, self.sum_keys):
            x.apply_galois(g, k0, k1, base_bits=W, out=rot)
            x.add(rot, out=x)
        x._call("zkfhe_bfv_cts_download", [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, self.u64p, self.u64p], None, x._handle(), 0, x.n,
                *[a.ctypes.data_as(self.u64p) for a in out])
        return out

    def batch(self, c0, c1, x, rot, out):
        x.store(c0, c1)
        return self.on_batch(x, rot, out)

    def close(self):
        self.plan.close()


def kernel_ms(ctx, zk, fn):
    ctx.prof_enable(True)   # resets the slots
    fn()
    prof = {s: ctx.prof_read(s) for s in range(zk.PROF_BFV_RESIDENT + 1)}
    ctx.prof_enable(False)
    return sum(p["total_ms"] for p in prof.values()), {s: [p["launches"], round(p["total_ms"], 4)] for s, p in prof.items() if p["launches"]}


def compare(ctx, zk, np, legs, reps, prof_reps):
    """legs: {"host": fn, "batch": fn}, each returning its two result arrays -> wall and kernel ms per leg (lists), and the slots of
    the last profiled pass"""
    res = {name: [a.copy() for a in fn()] for name, fn in legs.items()}   # warm-up: tables, arena, code objects
    assert all(np.array_equal(a, b) for a, b in zip(res["host"], res["batch"])), "the two chains differ"
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
        for count in CTS:
            c0 = rng.integers(0, q, size=(count, n), dtype=np.uint64)   # the cost does not depend on the values
            c1 = rng.integers(0, q, size=(count, n), dtype=np.uint64)
            host, x, rot = chain.buffers(count)
            out = [np.zeros((count, n), dtype=np.uint64) for _ in range(2)]
            legs = {"host": lambda: chain.host(c0, c1, host), "batch": lambda: chain.batch(c0, c1, x, rot, out)}
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

    row = row_of("box_tally_chain", prm, 3, *compare(ctx, zk, np, {"host": through_host, "batch": on_device}, a.reps, a.prof_reps))
    x.close(), rot.close(), box.close(), chain.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prof-reps", type=int, default=3)
    ap.add_argument("--box", action="store_true", help="also the chain on the tally of a ballot box of 3 groups (makes six k = 13 proofs)")
    a = ap.parse_args()
    rows = measure(a)
    rng_of = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])  # noqa: E731
    print("\n| chain | N | Q bits | ciphertexts | wall ms host arrays: median (min .. max) of %d | wall ms batch | host / batch | kernel ms host arrays: median (min .. max) of %d | "
          "kernel ms batch | host / batch |\n|---|---|---|---|---|---|---|---|---|---|" % (a.reps, a.prof_reps))
    for r in rows:
        print("| %s | %d | %d | %d | %s | %s | %.2f | %s | %s | %.3f |" % (
            r["what"], r["N"], r["Q"].bit_length(), r["cts"], rng_of(r["host"]["wall_ms"]), rng_of(r["batch"]["wall_ms"]), r["wall_ratio"],
            rng_of(r["host"]["kernel_ms"]), rng_of(r["batch"]["kernel_ms"]), r["kernel_ratio"]))


if __name__ == "__main__":
    main()
