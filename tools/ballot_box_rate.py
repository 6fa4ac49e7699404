"""The ballot box (zkfhe_bfv_box_add) against its two hand-written equivalents on the same inputs, in one process.  N distinct k = 13
Poseidon proofs of zk_fhe_amd.inputs under ONE public key (distinct ciphertexts: a repeat would not be counted), and per repetition,
interleaved:

    (a) verify       zk.bfv_verify_batch alone
    (b) by hand      zk.bfv_verify_batch, numpy extraction of the accepted c0 | c1 words from the instance bytes, ctx.bfv_sum
    (c) box          BallotBox.add on a fresh box (creation not timed), and add + tally

One JSON line with the minimum and the median wall time of each over the repetitions, the kernel time of one add by the profiler
(its own run), and a markdown table row.

    python tools/ballot_box_rate.py [--proofs 256] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    from oracle import circuit_ref as C
    os.environ.setdefault("ZKFHE_TABLE_GB", "4")
    cfgj = json.load(open(os.path.join(ROOT, "tests", "golden", "bfv", "bfv_config.json")))
    prm = C.BfvParams()
    n, params = 1024, (1024, prm.Q, prm.T, prm.B)
    ctx = zk.Context(0)
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(n)), params, zk.BfvConfig.from_pinning(cfgj), replay=True)
    vk = pk.export_vk()
    items = []
    for j in range(a.proofs):
        proof, inst, _ = pk.prove(json.dumps(inputs.generate(n, prm.Q, prm.T, prm.B, seed=5000 + j, key_seed=0)), b"box-%d" % j)
        items.append((inst, proof))
    pk.destroy()
    srs.destroy()
    pk0, pk1, _, _ = zk.bfv_instance_words(params, items[0][0])

    def verify():
        return zk.bfv_verify_batch(ctx, vk, items)

    def by_hand():
        res = zk.bfv_verify_batch(ctx, vk, items)
        words = np.stack([np.frombuffer(inst.raw, dtype=np.uint64).reshape(-1, 4)[2 * n:4 * n, 0] for (inst, _), (ok, _) in zip(items, res) if ok])
        return ctx.bfv_sum(params, words[:, :n], words[:, n:])

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    box = zk.BallotBox(ctx, vk, params, pk0, pk1)            # warm-up of every leg: code objects, allocators, work arenas
    assert all(s == zk.BALLOT_COUNTED for s, _ in box.add(items))
    want = by_hand()
    got = box.tally()
    assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[1][0], want[1]) and int(got[2][0]) == a.proofs
    box.close()
    verify()
    t = {"verify": [], "by_hand": [], "box_add": [], "box_add_tally": []}
    for _ in range(a.reps):
        t["verify"].append(timed(verify)[0])
        t["by_hand"].append(timed(by_hand)[0])
        box = zk.BallotBox(ctx, vk, params, pk0, pk1)
        ms_add, res = timed(lambda: box.add(items))
        ms_tally, _ = timed(box.tally)
        assert all(s == zk.BALLOT_COUNTED for s, _ in res)
        t["box_add"].append(ms_add)
        t["box_add_tally"].append(ms_add + ms_tally)
        box.close()
    # the kernels of one add, in a run of their own (profiling serialises the stream)
    box = zk.BallotBox(ctx, vk, params, pk0, pk1)
    ctx.prof_enable(True)
    box.add(items)
    kern = ctx.prof_read(zk.PROF_BFV_BALLOT)
    ctx.prof_enable(False)
    box.close()
    out = {"n_proofs": a.proofs, "reps": a.reps}
    for k, v in t.items():
        out[k + "_ms_min"], out[k + "_ms_median"] = round(min(v), 2), round(statistics.median(v), 2)
    out["ballot_kernels_ms"], out["ballot_kernel_launches"] = round(kern["total_ms"], 4), kern["launches"]
    print(json.dumps(out), flush=True)
    print("| %d | %s |" % (a.proofs, " | ".join("%.1f / %.1f" % (min(v), statistics.median(v)) for v in t.values())), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
