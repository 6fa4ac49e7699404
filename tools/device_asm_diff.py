#!/usr/bin/env python3
"""Is the gfx950 device code of two trees the same?  With no GPU.

Compiles every unit of build.units() of both trees (the -DZK_TILE_LOGN=k variants included) to device assembly with that tree's own
build.FLAGS, drops the lines that name the __hip_cuid_ symbol (a hash of the source text) and compares what is left line by line.  A
refactor of the headers that leaves every unit identical cannot have changed what the GPU runs, nor its speed.

    python tools/device_asm_diff.py ../parent-checkout .          # exit status 0: every unit identical

Host-only units (.cpp) have no device pass and are skipped.
"""
import argparse
import concurrent.futures as cf
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from count_addition_path import compile_to_asm


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a", help="repository root of the first tree (e.g. a checkout of the parent commit)")
    ap.add_argument("tree_b", help="repository root of the second tree")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    a = ap.parse_args()
    A, B = device_asm(a.tree_a, a.jobs), device_asm(a.tree_b, a.jobs)
    differ = 0
    for name in sorted(set(A) | set(B)):
        if name not in A or name not in B:
            print("%-24s only in %s" % (name, a.tree_a if name in A else a.tree_b))
            differ += 1
        elif A[name] == B[name]:
            print("%-24s identical (%d lines)" % (name, len(A[name])))
        else:
            i = next((i for i, (x, y) in enumerate(zip(A[name], B[name])) if x != y), min(len(A[name]), len(B[name])))
            print("%-24s DIFFERS at line %d (%d against %d lines)" % (name, i + 1, len(A[name]), len(B[name])))
            print("    a: %s\n    b: %s" % (A[name][i] if i < len(A[name]) else "<end>", B[name][i] if i < len(B[name]) else "<end>"))
            differ += 1
    print("%d unit(s), %d differ" % (len(set(A) | set(B)), differ))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
