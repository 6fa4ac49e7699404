"""BFV encryption rate on the GPU (zkfhe_bfv_encrypt) against the host generator (zk_fhe_amd.inputs.generate), and the input
stage of a proof from machine words (prove_words) against the JSON path (prove).  One JSON line per measurement:

  {"what": "encrypt", N, Q, batch, ms_per_call, enc_per_s, kernel_ms: {sample, rns_ntt, epilogue}}   (kernels: a separate profiled pass)
  {"what": "inputs.generate", N, Q, ms}                                                                   (host numpy, one input)
  {"what": "prove_input_stage", k, path, witness_ms, phase0_commit_ms, total_ms}                          (timings_ms + proof marks)

    python tools/bfv_encrypt_rate.py [--batches 1,8,64] [--reps 20] [--no-compare]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 536870909, 7), (4096, (1 << 60) - 93, 65537), (16384, (1 << 60) - 93, 65537)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-compare", action="store_true", help="skip the k = 13 prove / prove_words comparison")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    os.environ.setdefault("ZKFHE_TABLE_GB", "4")
    ctx = zk.Context(0)
    rng = np.random.default_rng(0)
    for n, q, t in SIZES:
        prm = (n, q, t, 19)
        _, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
        for batch in [int(x) for x in a.batches.split(",")]:
            m = np.array([int(x) % q for x in rng.integers(-(t // 2), t // 2 + 1, batch * n)], dtype=np.uint64).reshape(batch, n)
            ctx.bfv_encrypt(prm, pk0, pk1, m)   # warm-up: tables, arena
            t0 = time.perf_counter()
            for _ in range(a.reps):
                ctx.bfv_encrypt(prm, pk0, pk1, m)
            ms = (time.perf_counter() - t0) * 1e3 / a.reps
            ctx.prof_enable(True)
            ctx.bfv_encrypt(prm, pk0, pk1, m)
            kern = {name: round(ctx.prof_read(slot)["total_ms"], 4) for name, slot in
                    (("sample", zk.PROF_BFV_SAMPLE), ("rns_ntt", zk.PROF_RNS_NTT), ("epilogue", zk.PROF_RNS_EPILOGUE))}
            ctx.prof_enable(False)
            print(json.dumps({"what": "encrypt", "N": n, "Q": q, "batch": batch, "ms_per_call": round(ms, 3),
                              "enc_per_s": round(batch * 1e3 / ms, 1), "kernel_ms": kern}), flush=True)
        t0 = time.perf_counter()
        inputs.generate(n, q, t, 19, seed=1)
        print(json.dumps({"what": "inputs.generate", "N": n, "Q": q, "ms": round((time.perf_counter() - t0) * 1e3, 1)}), flush=True)
    if not a.no_compare:
        from oracle import circuit_ref as C
        cfgj = json.load(open(os.path.join(ROOT, "tests", "golden", "bfv", "bfv_config.json")))
        p = C.BfvParams()
        prm = (1024, p.Q, p.T, p.B)
        srs = zk.Srs(ctx, 13)
        pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), prm, zk.BfvConfig.from_pinning(cfgj), replay=True)
        _, pk0, pk1 = ctx.bfv_fhe_keypair(prm, os.urandom(32))
        m = np.zeros((1, 1024), dtype=np.uint64)
        ct = ctx.bfv_encrypt(prm, pk0, pk1, m)
        words = {"pk0": pk0, "pk1": pk1, "m": m[0], "u": ct["u"][0], "e0": ct["e0"][0], "e1": ct["e1"][0], "c0": ct["c0"][0], "c1": ct["c1"][0]}
        st = lambda v: [str(int(x)) for x in v]  # noqa: E731
        text = json.dumps({k: st(v) for k, v in words.items()} | {"cyclo": st([1] + [0] * 1023 + [1])})
        pk.prefix_cache(0)   # every proof hashes its whole public input: the two paths differ only in how the input arrives
        for path in ("prove", "prove_words") * 6:
            tm = pk.prove(text, b"cmp")[2] if path == "prove" else pk.prove_words(words, b"cmp")[2]
            marks = ctx.last_proof_marks()
            print(json.dumps({"what": "prove_input_stage", "k": 13, "path": path, "witness_ms": round(tm[0], 3),
                              "phase0_commit_ms": round(marks[0], 3), "total_ms": round(tm[4], 3)}), flush=True)
        pk.destroy()
        srs.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
