#!/usr/bin/env python3
"""What every command of a proof's chain costs the proof, from a rocprofv3 rocpd database (kernel-trace) of a run with several
proofs in flight: per kernel name the calls, the average run time and the WAIT -- from the end of the previous command on the
same stream to this command's start.  The median wait is what a command in the middle of a round spends queued behind other
proofs' commands (alone it is 0); the mean also holds the host's time at the head of every Fiat-Shamir round.
usage: tools/chain_latency.py <results.db> [proofs]      (proofs: divide the calls by this many; default: count of k_sh_w)"""
import collections
import sqlite3
import sys


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][-40:]


def main():
    db = sqlite3.connect(sys.argv[1])
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    key = "stream_id" if "stream_id" in cols else ("stream" if "stream" in cols else "queue_id")
    rows = db.execute("select name, start, duration, %s from kernels order by start" % key).fetchall()
    proofs = int(sys.argv[2]) if len(sys.argv) > 2 else max(1, sum(1 for r in rows if "k_sh_w" in r[0]))
    prev_end = {}
    agg = collections.defaultdict(lambda: [0, 0.0, []])
    for name, start, dur, stream in rows:
        n = short(name)
        if stream in prev_end:
            agg[n][2].append(max(0.0, (start - prev_end[stream]) / 1e3))
        agg[n][0] += 1
        agg[n][1] += dur / 1e3
        prev_end[stream] = max(prev_end.get(stream, 0), start + dur)
    print("streams keyed by `%s`: %d; proofs: %d" % (key, len(prev_end), proofs))
    print("| command | calls per proof | avg run us | median wait us | mean wait us | (run + median wait) per proof us |")
    print("|---|---|---|---|---|---|")

    def per_proof(v):
        c, run, waits = v
        med = sorted(waits)[len(waits) // 2] if waits else 0.0
        return c / proofs * (run / c + med)
    for n, v in sorted(agg.items(), key=lambda kv: -per_proof(kv[1])):
        c, run, waits = v
        med = sorted(waits)[len(waits) // 2] if waits else 0.0
        print("| %s | %.2f | %.1f | %.1f | %.1f | %.0f |" % (n, c / proofs, run / c, med, sum(waits) / max(1, len(waits)), per_proof(v)))


if __name__ == "__main__":
    main()
