#!/usr/bin/env python3
"""Static instruction count of the point-addition loop of an MSM kernel, with no GPU.

Compiles a translation unit to gfx950 assembly with build.py's flags (or reads an assembly file made that way) and prints, for the
named kernel, the instruction classes of the COMMON PATH of its addition loop, and VGPRs, scratch bytes and occupancy from the
compiler's resource summary of the kernel.

    python tools/count_addition_path.py zk-fhe_amd/csrc/msm.hip 'k_msm_table<false>'
    python tools/count_addition_path.py --asm msm.s 'k_msm_table<false>'          # an assembly file kept from another tree

The loop: the shortest backward branch range of the kernel that holds at least --min-mads 64-bit multiply-adds; the default is the 1467
of one mixed addition's nine products (six mul of 162, two sqr of 126, one fused two-product of 243).  The common path: of all the ways
through that range from its first block to its backward branch (forward edges only) that have at least that many multiply-adds, the
one with the fewest instructions -- the full addition and nothing else; the empty-accumulator, identity-entry, doubling and cancellation
paths have fewer products, and a way that runs through the doubling AND the addition is longer.  Blocks the compiler moved behind the
loop (rare paths) are not followed.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-fhe_amd"))

MEM = ("global_", "flat_", "scratch_", "buffer_", "ds_")
CLASSES = ["mad64", "shift64", "v_mul_lo", "v_and", "lane_moves", "other_valu", "s_nop", "scalar", "memory"]


def classify(op):
    if op in ("v_mad_u64_u32", "v_mad_i64_i32"):
        return "mad64"
    if op in ("v_lshrrev_b64", "v_ashrrev_i64"):
        return "shift64"
    if op.startswith("v_mul_lo_"):
        return "v_mul_lo"
    if op.startswith("v_and_b32"):
        return "v_and"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane_moves"
    if op.startswith("v_"):
        return "other_valu"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(MEM):
        return "memory"
    return "scalar"


def compile_to_asm(src, extra, build=None):
    """build: the build.py module whose flags to use (another tree's, for tools/device_asm_diff.py); this tree's by default"""
    if build is None:
        import build
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [build.hipcc()] + build.FLAGS + extra + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return names
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines()
    return out if len(out) == len(names) else names


def kernel_text(lines, want):
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m]
    nice = demangle([n for _, n in starts])
    def short(d):   # "void (anonymous namespace)::k<false>(args)" -> "k<false>"
        return re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "").replace("zk::", "").split("(")[0]
    hits = [(i, n, d) for (i, n), d in zip(starts, nice) if want in short(d) or want in n]
    exact = [h for h in hits if short(h[2]) == want]
    hits = exact or hits
    if len(hits) != 1:
        sys.exit("kernel %r: %d matches: %s" % (want, len(hits), [h[2] for h in hits][:8]))
    i0 = hits[0][0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    res = {}
    for l in lines[i1:i1 + 60]:
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|NumSgprs|codeLenInByte)\s*[:=]\s*(\d+)", l)
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
    return hits[0][2], lines[i0 + 1:i1], res


def blocks_of(body):
    """[(label, [ops], [branch targets], falls_through)]"""
    blocks, cur = [], ["<entry>", [], [], True]
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append(cur)
            cur = [m.group(1), [], [], True]
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        op = t.split()[0]
        cur[1].append(op)
        if op.startswith("s_cbranch") or op == "s_branch":
            cur[2].append(t.split()[-1])
            if op == "s_branch":
                cur[3] = False
            blocks.append(cur)   # what follows a branch is a block of its own, label or not
            cur = ["%s+%d" % (cur[0].split("+")[0], len(blocks)), [], [], True]
        if op in ("s_endpgm", "s_setpc_b64"):
            cur[3] = False
    blocks.append(cur)
    return blocks


def common_path(blocks, min_mads):
    idx = {b[0]: i for i, b in enumerate(blocks)}
    mads = [sum(1 for o in b[1] if classify(o) == "mad64") for b in blocks]
    best = None
    for i, b in enumerate(blocks):
        for t in b[2]:
            j = idx.get(t)
            if j is not None and j <= i and sum(mads[j:i + 1]) >= min_mads and (best is None or i - j < best[1] - best[0]):
                best = (j, i)
    if best is None:
        sys.exit("no loop with at least %d multiply-adds" % min_mads)
    lo, hi = best
    # every way through [lo, hi] over forward edges; of those with a full addition's multiply-adds, the shortest
    succ = {}
    for i in range(lo, hi + 1):
        out = [idx[t] for t in blocks[i][2] if t in idx] + ([i + 1] if blocks[i][3] else [])
        succ[i] = sorted(set(s for s in out if i < s <= hi))
    best_path, stack = None, [[lo]]
    while stack:
        path = stack.pop()
        if path[-1] == hi:
            if sum(mads[i] for i in path) >= min_mads:
                size = sum(len(blocks[i][1]) for i in path)
                if best_path is None or size < best_path[0]:
                    best_path = (size, path)
            continue
        for s in succ[path[-1]]:
            stack.append(path + [s])
    if best_path is None:
        sys.exit("no way through the loop with at least %d multiply-adds" % min_mads)
    return lo, hi, best_path[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a .hip translation unit, or with --asm a gfx950 assembly file")
    ap.add_argument("kernel", help="kernel name as written, e.g. 'k_msm_table<false>'")
    ap.add_argument("--asm", action="store_true", help="source is assembly already")
    ap.add_argument("--keep", help="keep the assembly under this name")
    ap.add_argument("--min-mads", type=int, default=1467)
    ap.add_argument("-D", action="append", default=[], help="extra define for the compile, e.g. -D ZK_MAD_C")
    a = ap.parse_args()
    path = a.source if a.asm else compile_to_asm(a.source, ["-D" + d for d in a.D])
    lines = open(path).read().splitlines()
    if not a.asm:
        if a.keep:
            shutil.copy(path, a.keep)
        os.unlink(path)
    name, body, res = kernel_text(lines, a.kernel)
    blocks = blocks_of(body)
    lo, hi, route = common_path(blocks, a.min_mads)
    cnt = dict.fromkeys(CLASSES, 0)
    for i in route:
        for o in blocks[i][1]:
            cnt[classify(o)] += 1
    whole = dict.fromkeys(CLASSES, 0)
    for b in blocks:
        for o in b[1]:
            whole[classify(o)] += 1
    valu = sum(cnt[c] for c in ("mad64", "shift64", "v_mul_lo", "v_and", "lane_moves", "other_valu"))
    print("kernel: %s" % name)
    print("loop: blocks %s .. %s, common path over %d of its %d blocks" % (blocks[lo][0], blocks[hi][0], len(route), hi - lo + 1))
    print("| per addition, common path | instructions | whole kernel |")
    print("|---|---|---|")
    for c in CLASSES:
        print("| %s | %d | %d |" % (c, cnt[c], whole[c]))
    print("| VALU (all v_*) | %d | |" % valu)
    print("| VALU slots (v_* + s_nop) | %d | |" % (valu + cnt["s_nop"]))
    print("| total | %d | %d |" % (sum(cnt.values()), sum(whole.values())))
    print("resources: " + ", ".join("%s %d" % kv for kv in sorted(res.items())))


if __name__ == "__main__":
    main()
