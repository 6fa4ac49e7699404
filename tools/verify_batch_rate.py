"""Batch verification rate (zkfhe_bfv_verify_batch) against the single host verifier on a pool of the usable CPUs, in one
process.  k = 13 Poseidon proofs of zk_fhe_amd.inputs under three public keys (64 distinct proofs, repeated to fill N).  One JSON
line per N: wall time and proofs/s, host CPU ms per proof (process_time over the call), GPU ms per stage (zkfhe_prof_*), and the
single verifier's rate over the same proofs (at most 256 of them).

    python tools/verify_batch_rate.py [--sizes 1,16,256,1024]
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def usable_cpus():
    n = len(os.sched_getaffinity(0))
    omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return min(n, omp) if omp > 0 else n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256,1024")
    ap.add_argument("--distinct", type=int, default=64)
    a = ap.parse_args()
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    from zk_fhe_amd import inputs
    from oracle import circuit_ref as C
    os.environ.setdefault("ZKFHE_TABLE_GB", "4")
    cfgj = json.load(open(os.path.join(ROOT, "tests", "golden", "bfv", "bfv_config.json")))
    prm = C.BfvParams()
    ctx = zk.Context(0)
    srs = zk.Srs(ctx, 13)
    pk = zk.BfvProvingKey(ctx, srs, json.dumps(inputs.empty(1024)), (1024, prm.Q, prm.T, prm.B), zk.BfvConfig.from_pinning(cfgj), replay=True)
    vk = pk.export_vk()
    base = []
    for j in range(a.distinct):
        proof, inst, _ = pk.prove(json.dumps(inputs.generate(1024, prm.Q, prm.T, prm.B, seed=1000 + j, key_seed=j % 3)), b"rate-%d" % j)
        base.append((inst, proof))
    pk.destroy()
    srs.destroy()
    cpus = usable_cpus()
    pool = cf.ThreadPoolExecutor(max_workers=cpus)   # the C verifier releases the GIL (ctypes)
    zk.bfv_verify_batch(ctx, vk, base[:2])           # warm-up: code objects, allocator
    for N in [int(x) for x in a.sizes.split(",")]:
        items = [base[j % len(base)] for j in range(N)]
        ctx.prof_enable(True)
        t0, c0 = time.perf_counter(), time.process_time()
        res = zk.bfv_verify_batch(ctx, vk, items)
        wall, cpu = time.perf_counter() - t0, time.process_time() - c0
        dec, seg = ctx.prof_read(zk.PROF_G1_DECOMPRESS), ctx.prof_read(zk.PROF_MSM_SEGMENTED)
        ctx.prof_enable(False)
        assert all(ok for ok, _ in res), res[:4]
        M = min(N, 256)
        t1, c1 = time.perf_counter(), time.process_time()
        single = list(pool.map(lambda it: zk.bfv_verify(vk, it[0], it[1]), items[:M]))
        swall, scpu = time.perf_counter() - t1, time.process_time() - c1
        assert all(ok for ok, _ in single)
        print(json.dumps({
            "n_proofs": N, "batch_wall_ms": round(wall * 1e3, 2), "batch_proofs_per_s": round(N / wall, 1),
            "batch_host_cpu_ms_per_proof": round(cpu * 1e3 / N, 3),
            "gpu_ms": {"k_g1_decompress": round(dec["total_ms"], 3), "k_msm_segmented": round(seg["total_ms"], 3)},
            "gpu_ms_per_proof": round((dec["total_ms"] + seg["total_ms"]) / N, 4),
            "single_pool_cpus": cpus, "single_proofs": M, "single_proofs_per_s": round(M / swall, 1),
            "single_host_cpu_ms_per_proof": round(scpu * 1e3 / M, 3),
        }), flush=True)
    pool.shutdown()
    ctx.close()


if __name__ == "__main__":
    main()
