#!/usr/bin/env python3
"""Is the gfx950 device code of two trees the same?  With no GPU.

Compiles every unit of build.units() of both trees (the -DZK_TILE_LOGN=k variants included) to device assembly with that tree's own
build.FLAGS, drops the lines that name the __hip_cuid_ symbol (a hash of the source text) and compares what is left line by line.  A
refactor of the headers that leaves every unit identical cannot have changed what the GPU runs, nor its speed.

    python tools/device_asm_diff.py ../parent-checkout .          # exit status 0: every unit identical

Host-only units (.cpp) have no device pass and are skipped.

A refactor that moves or renames kernels changes their units.  --pairs looks into the units that differ, kernel by kernel:

    python tools/device_asm_diff.py ../parent-checkout . --pairs 'k_old<true> = k_new<Src>' 'k_other = k_other2'

For each pair it compares the instruction count per mnemonic and the kernel descriptor's VGPR, SGPR, LDS and scratch figures (so a
different register numbering or instruction order passes, a different count does not).  Every other kernel of those units must
exist under its name in both trees, whichever unit holds it, with an identical body (block labels are numbered per unit and compared
without their numbers) or at least with equal counts and figures, which is reported as such.  Exit status 0: nothing else differs.
"""
import argparse
import collections
import concurrent.futures as cf
import importlib.util
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from count_addition_path import compile_to_asm, demangle

FIGURES = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr", "lds": ".amdhsa_group_segment_fixed_size",
           "scratch": ".amdhsa_private_segment_fixed_size"}


def load_build(tree):
    path = os.path.join(os.path.abspath(tree), "zk-fhe_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(tree, jobs):
    """{unit name: assembly lines without the __hip_cuid_ ones} of every unit of the tree that has a device pass"""
    build = load_build(tree)
    todo = [(os.path.basename(obj)[:-2], src, extra) for src, obj, extra in build.units() if not src.endswith(".cpp")]

    def one(t):
        name, src, extra = t
        path = compile_to_asm(src, extra, build)
        lines = [l for l in open(path).read().splitlines() if "__hip_cuid_" not in l]
        os.unlink(path)
        return name, lines

    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        return dict(ex.map(one, todo))


def short_name(d):
    """ "void (anonymous namespace)::k<zkrns::S>(args)" -> "k<S>" """
    return re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "").replace("zkrns::", "").replace("zk::", "").split("(")[0]


def kernels(lines):
    """{short name: (instructions with block labels unnumbered, descriptor figures)} of the kernels of one unit's assembly"""
    desc, cur = {}, None
    for l in lines:
        t = l.split()
        if t[:1] == [".amdhsa_kernel"]:
            cur = desc.setdefault(t[1], {})
        elif t[:1] == [".end_amdhsa_kernel"]:
            cur = None
        elif cur is not None:
            for k, v in FIGURES.items():
                if t[:1] == [v]:
                    cur[k] = int(t[1])
    names = list(desc)
    out = {}
    for sym, nice in zip(names, demangle(names)):
        i0 = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = []
        for l in lines[i0 + 1:i1]:
            t = re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0]).strip()
            if t and not (t.startswith(".") and not t.endswith(":")):
                body.append(" ".join(t.split()))
        out[short_name(nice)] = (body, desc[sym])
    return out


def histogram(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def compare_kernels(A, B, units, pairs):
    """the kernels of `units` in both trees: the pairs by histogram and figures, the rest by name and body.  Returns what differs."""
    old, new = collections.defaultdict(list), collections.defaultdict(list)
    for pool, tree in ((old, A), (new, B)):
        for u in units:
            for name, k in kernels(tree.get(u, [])).items():
                pool[name].append(k)
    differ = 0
    for a, b in pairs:
        if len(old.get(a, [])) != 1 or len(new.get(b, [])) != 1:
            print("  %-44s = %-44s MISSING (%d old, %d new)" % (a, b, len(old.get(a, [])), len(new.get(b, []))))
            differ += 1
            continue
        (ba, fa), (bb, fb) = old.pop(a)[0], new.pop(b)[0]
        ha, hb = histogram(ba), histogram(bb)
        fig = ", ".join("%s %d" % (k, fa[k]) if fa[k] == fb[k] else "%s %d -> %d" % (k, fa[k], fb[k]) for k in FIGURES)
        if ha == hb and fa == fb:
            print("  %-44s = %-44s equal: %d instructions, %s%s" % (a, b, sum(ha.values()), fig, "" if ba == bb else " (order or registers differ)"))
        else:
            diff = ", ".join("%s %d -> %d" % (m, ha[m], hb[m]) for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m])
            print("  %-44s = %-44s DIFFERS: %d -> %d instructions, %s; %s" % (a, b, sum(ha.values()), sum(hb.values()), fig, diff or "-"))
            differ += 1
    for name in sorted(set(old) | set(new)):
        ks = old.get(name, []) + new.get(name, [])
        if name not in old or name not in new:
            print("  %-44s only in the %s tree" % (name, "first" if name in old else "second"))
            differ += 1
        elif all(k == ks[0] for k in ks):
            print("  %-44s identical body (%d instructions, scratch %d)" % (name, sum(histogram(ks[0][0]).values()), ks[0][1]["scratch"]))
        elif all(histogram(k[0]) == histogram(ks[0][0]) and k[1] == ks[0][1] for k in ks):   # e.g. a header's kernel beside other neighbours
            print("  %-44s equal counts and figures, order or registers differ (%d instructions, scratch %d)"
                  % (name, sum(histogram(ks[0][0]).values()), ks[0][1]["scratch"]))
        else:
            print("  %-44s DIFFERS" % name)
            differ += 1
    return differ


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a", help="repository root of the first tree (e.g. a checkout of the parent commit)")
    ap.add_argument("tree_b", help="repository root of the second tree")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--pairs", nargs="+", default=[], metavar="'OLD = NEW'",
                    help="kernels of tree_a and what they are called in tree_b, names as written, e.g. 'k_switch<true> = k_switch<Galois>'")
    a = ap.parse_args()
    pairs = [tuple(x.strip() for x in p.split(" = ")) for p in a.pairs]
    A, B = device_asm(a.tree_a, a.jobs), device_asm(a.tree_b, a.jobs)
    differ, changed = 0, []
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            print("%-24s only in %s" % (name, a.tree_a if name in A else a.tree_b))
            differ += 1
            changed.append(name)
        elif A[name] == B[name]:
            print("%-24s identical (%d lines)" % (name, len(A[name])))
        else:
            i = next((i for i, (x, y) in enumerate(zip(A[name], B[name])) if x != y), min(len(A[name]), len(B[name])))
            print("%-24s DIFFERS at line %d (%d against %d lines)" % (name, i + 1, len(A[name]), len(B[name])))
            print("    a: %s\n    b: %s" % (A[name][i] if i < len(A[name]) else "<end>", B[name][i] if i < len(B[name]) else "<end>"))
            differ += 1
            changed.append(name)
    print("%d unit(s), %d differ" % (len(set(A) | set(B)), differ))
    if pairs and changed:
        print("the kernels of %s:" % ", ".join(changed))
        differ = compare_kernels(A, B, changed, pairs)
        print("%d kernel(s) differ" % differ)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
