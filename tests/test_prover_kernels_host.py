"""The CPU half of tests/test_gpu_prover_kernels.py: the Python references of tests/prover_kernel_cases.py against other statements of
the same operations (inverse NTT and Horner through the C oracle, a plain product, polynomial division), the case list itself -- every
edge it is meant to hold is there -- and a compile of the driver for gfx950."""
import os
import random
import shutil
import subprocess
import time

import pytest

from oracle import binding as orc
from tests import prover_kernel_cases as pc
from tests.prover_kernel_cases import ONE, R, SENT, W, mulw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cases():
    t0 = time.time()
    c = pc.build()
    print("prover kernel cases: %d launches, references in %.1f s" % (sum(l.startswith("run ") for l in c.lines), time.time() - t0))
    return c


# ------------------------------------------------------------------------------------------------ the references
def test_conventions():
    assert SENT >= R and pc.to_bytes([SENT]) == b"\xa5" * 32
    assert mulw(W(3), W(5)) == W(15) and pc.mul29(W(3), 5 * (1 << 261) % R) == W(15)
    assert pc.invw(0) == 0 and mulw(pc.invw(W(7)), W(7)) == ONE
    assert len(set(pc.EDGE)) == pc.M >= 18 and {0, 1, R - 1} <= set(pc.EDGE) and all(0 <= w < R for w in pc.EDGE)


def test_evaluation_reference_against_inverse_ntt_and_horner():
    """with the barycentric weights (z^n - 1) / n * w^i / (z - w^i) in the 2^261 form, sum_i col[i] bw[i] 2^-261 is the word of p(z), p
    the polynomial of degree < n with p(w^i) = col[i]: the oracle's inverse NTT and Horner rule"""
    rnd = random.Random(5)
    n = 512
    col = [rnd.randrange(R) for _ in range(n)]
    coeffs = orc.ntt(orc.ints_to_arr(col).reshape(1, n, 4), 9, inverse=True)[0]
    for z in (rnd.randrange(R), 2, R - 2):
        c = (pow(z, n, R) - 1) * pow(n, -1, R) % R
        wi = [pow(pc.OMEGA9, i, R) for i in range(n)]
        bw = [c * w % R * pow(z - w, -1, R) % R * (1 << 261) % R for w in wi]
        want = orc.arr_to_ints(orc.fr_horner(coeffs, orc.ints_to_arr([W(z)])[0]).reshape(1, 4))[0]
        assert pc.ref_eval(col, bw) == want
        assert (pc.ref_eval(col, bw, 0, 200) + pc.ref_eval(col, bw, 200, n)) % R == want


def test_prefix_reference_is_the_product_of_the_ratios():
    rnd = random.Random(6)
    vals = [rnd.randrange(R) for _ in range(40)]
    for u in (0, 1, 39):
        z = pc.ref_prefix([W(v) for v in vals], u)
        assert len(z) == u + 1 and z[0] == ONE
        p = 1
        for v in vals[:u]:
            p = p * v % R
        assert z[u] == W(p)


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


def poly_divmod(a, b):
    a, q = list(a), [0] * max(1, len(a) - len(b) + 1)
    inv = pow(b[-1], -1, R)
    for k in range(len(a) - len(b), -1, -1):
        q[k] = a[k + len(b) - 1] * inv % R
        for j, y in enumerate(b):
            a[k + j] = (a[k + j] - q[k] * y) % R
    return q, a[:len(b) - 1]


def poly_eval(a, x):
    acc = 0
    for v in reversed(a):
        acc = (acc * x + v) % R
    return acc


def interpolate(xs, ys):
    out = [0]
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num, den = [1], 1
        for j, xj in enumerate(xs):
            if j != i:
                num, den = poly_mul(num, [-xj % R, 1]), den * (xi - xj) % R
        s = yi * pow(den, -1, R) % R
        out = [(a + s * b) % R for a, b in zip(out + [0] * (len(num) - len(out)), num)]
    return out


def test_shplonk_references_against_polynomial_division():
    """n = 8, three rotation sets: h = sum_j v^j (F_j - r_j) / Z_Sj and W = (sum_j v^j Z_{T \\ Sj}(u) (F_j - r_j(u)) - Z_T(u) h) / (X - u) by long
    division (no remainder), evaluated on the domain, against k_sh_zs / k_sh_h / k_sh_w's references on the evaluations"""
    rnd = random.Random(7)
    log_n, n = 3, 8
    omega = pc.pyref.root_of_unity(log_n)
    dom = [pow(omega, i, R) for i in range(n)]
    v, u = rnd.randrange(R), rnd.randrange(R)
    T = [rnd.randrange(R) for _ in range(4)]
    S = [T[:1], T[1:3], T]
    F = [[rnd.randrange(R) for _ in range(n)] for _ in S]   # coefficients
    h, L, sets, coef, r_u = [0], [0], [], [], []
    for j, (s, f) in enumerate(zip(S, F)):
        rj = interpolate(s, [poly_eval(f, x) for x in s])
        zs = [1]
        for x in s:
            zs = poly_mul(zs, [-x % R, 1])
        q, rem = poly_divmod([(a - b) % R for a, b in zip(f, rj + [0] * n)], zs)
        assert not any(rem)
        vj = pow(v, j, R)
        h = [(a + vj * b) % R for a, b in zip(h + [0] * n, q + [0] * n)][:n]
        zrest = 1
        for x in T:
            if x not in s:
                zrest = zrest * (u - x) % R
        coef.append(vj * zrest % R)
        r_u.append(poly_eval(rj, u))
        L = [(a + coef[-1] * b) % R for a, b in zip(L + [0] * n, [(f[0] - r_u[-1]) % R] + f[1:])][:n]
        sets.append(dict(rc=[W(x) for x in rj + [0] * (4 - len(rj))], vj=W(vj), pts=[W(x) for x in s]))
    ztu = 1
    for x in T:
        ztu = ztu * (u - x) % R
    L = [(a - ztu * b) % R for a, b in zip(L, h)]
    Wq, rem = poly_divmod(L, [-u % R, 1])
    assert not any(rem)
    wpow = [W(x) for x in dom]
    Fe = [[W(poly_eval(f, x)) for x in dom] for f in F]
    zs_inv = [[pc.invw(pc.ref_sh_zs(s["pts"], w)) for w in wpow] for s in sets]
    hq = pc.ref_sh_h(sets, Fe, zs_inv, wpow)
    assert hq == [W(poly_eval(h, x)) for x in dom]
    inv = [pc.invw((w - W(u)) % R) for w in wpow]
    got = pc.ref_sh_w([W(x) for x in coef], [W(x) for x in r_u], Fe, hq, W(ztu), inv)
    assert got == [W(poly_eval(Wq, x)) for x in dom]


def test_rng_rows_are_the_oracle_stream():
    from oracle import halo2_ref as H
    g = H.Rng(b"seed")
    draws = g.take(12)
    assert pc.rng_row_words(b"seed", 9, 3) == [W(x) for x in draws[9:12]]


# ------------------------------------------------------------------------------------------------ the case list
def runs(c, kernel):
    return [l.split() for l in c.lines if l.startswith("run ") and l.split()[2] == kernel]


def test_every_buffer_argument_names_a_declared_buffer_and_every_check_is_dumped(cases):
    declared = {l.split()[1]: int(l.split()[2]) for l in cases.lines if l.startswith("buf ")}
    dumped = {l.split()[1] for l in cases.lines if l.startswith("dump ")}
    assert all(size > 0 for size in declared.values())
    for g in pc.GROUPS:
        for case, buf, want, mask in cases.checks[g]:
            assert buf in dumped and len(want) == declared[buf], (case, buf)
    for l in cases.lines:
        if l.startswith("run "):
            for tok in l.split()[3:]:
                if tok[0] == "b":
                    name, _, off = tok.partition("+")
                    assert name in declared and int(off or 0) < declared[name], l[:80]
    names = [l.split()[1] for l in cases.lines if l.startswith("run ")]
    assert len(names) == len(set(names))
    assert max(len(v) for v in cases.files.values()) <= 6 * 32 * (1 << 17)


def test_permutation_cases(cases):
    f = cases.facts["perm"]
    n = pc.N
    assert (f["n_adv"], f["n_perm"]) == (5, 7)
    assert sorted(int(r[7]) for r in runs(cases, "perm")) == [1, 1, 3, 3, 7, 7]   # chunk; 3: columns 3, 3 and 1 -- advice and constants meet in the second
    assert {int(r[3]) for r in runs(cases, "perm")} == {1, 2, pc.blocks(3 * n), pc.blocks(7 * n)}
    for chunk in (3, 7, 1):
        num, den = f["chunk%d" % chunk]
        for arr, planted in ((num, f["num_zero"]), (den, f["den_zero"])):
            assert {i for i, x in enumerate(arr) if x == 0} == {(k // chunk) * n + row for k, row in planted}   # zero there and only there
    cols = {k for k, _ in f["num_zero"] + f["den_zero"]}
    assert 5 in cols and 6 in cols and min(cols) < 5   # the constants, the instance, an advice column


def test_lookup_cases(cases):
    assert sorted({(d["nl"], d["beta"] == R - 1, d["beta"] == 0) for d in cases.facts["lookup"]}) == sorted(
        {(nl, a, b) for nl in (1, 3) for a, b in ((False, False), (True, False), (False, True))})
    for d in cases.facts["lookup"]:
        assert d["beta"] == d["gamma"] or d["beta"] not in (0, R - 1)
        for l in range(d["nl"]):
            assert any((x + d["beta"]) % R == 0 for x in d["a"][l]) and any((x + d["beta"]) % R == 0 for x in d["la"][l])
            assert any((x + d["gamma"]) % R == 0 for x in d["ls"][l])
            for col in (d["a"][l], d["la"][l], d["ls"][l], d["table"]):
                assert {0, 255, R - 1, W(255), W(R - 1)} <= set(col)
        assert any((x + d["gamma"]) % R == 0 for x in d["table"])
        assert 0 in d["num"] and 0 in d["den"]


def test_prefix_cases(cases):
    seen = {}
    for d in cases.facts["prefix"]:
        n, u, per = d["n"], d["u"], d["per"]
        assert per == -(-n // 1024) and 0 < d["boundary"] < u - 1 and d["boundary"] % per == 0 and u < n
        seen.setdefault(n, []).append(u)
        z = d["zfull"]
        assert set(z["ones"]) == {ONE} and z["minus_one"][:3] == [ONE, W(R - 1), ONE]
        assert z["zero_row0"][0] == ONE and not any(z["zero_row0"][1:])
        b = d["boundary"]
        assert all(z["zero_boundary"][:b + 1]) and not any(z["zero_boundary"][b + 1:])   # everything after the zero is 0, nothing before it
        zl, p1 = d["ucols"]["zero_last"][1], d["ucols"]["product_one"][1]
        assert len(zl) == len(p1) == u + 1 and all(zl[:u]) and zl[u] == 0 and p1[u] == ONE and p1[u - 1] != ONE
        assert pc.ref_prefix(d["ucols"]["product_one"][0], u) == p1
    assert sorted(seen) == [512, 1024, 2048, 65536]
    for n, us in seen.items():
        per = -(-n // 1024)
        assert (n - 7 if n == 512 else n - 107) in us and n - 1 in us
        assert any(u % per == 0 and u - 1 in us and u + 1 in us for u in us)   # z[u] the first row of a thread, the last, the second
    b = cases.facts["prefix_blind"]
    assert b["ctr0"] > 0 and b["stride"] > b["n"] - b["u"] - 1 > 0
    assert [r for r in runs(cases, "prefix") if r[9] == "1"][0][5] == "3"   # blinding on: three columns


def test_prefix_segment_cases(cases):
    f = cases.facts["prefix_seg"]
    assert [d["u"] for d in f] == [(1 << 17) - 107, (1 << 17) - 1, 3 * 32768]
    for d in f:
        assert d["n"] == 1 << 17 and d["n"] // d["seg_len"] == 4
        zero_at = {k: v.index(0) for k, v in d["cols"].items() if 0 in v}
        assert zero_at == {"zero_boundary": 2 * 32768, "zero_seg0": 5}
        assert d["ucols"]["zero_last"][0].index(0) == d["u"] - 1 >= 3 * 32768 - 1
    seg, one = runs(cases, "prefix_seg"), [r for r in runs(cases, "prefix") if r[1].endswith("_one_workgroup")]
    assert len(seg) == len(one) == 12 and all(r[5] == "2" for r in seg)
    assert [r[7] for r in seg] == [r[6] for r in one]   # the same inputs through both


def test_chunk_carry_cases(cases):
    f = cases.facts["carry"]
    assert sorted({c for c, _, _ in f}) == [1, 3, 4, 5, 1023, 1024, 1025, 4096]
    for count, name, totals in f:
        assert len(totals) == count >= 1
        p = pc.ref_prefix(totals, count)[count]
        assert {"closes": p == ONE, "doubled": p == 2 * ONE % R, "zero": p == 0 and totals[count // 2] == 0}[name]
    g = cases.facts["carry_ones"]
    assert all(count >= 1 for count, _, _, _ in g)
    assert {name for _, name, _, _ in g} == {"all_ones", "first", "last", "second_slot"}
    assert all(spot == per + 1 and per >= 2 for _, name, spot, per in g if name == "second_slot")
    assert all(spot == count - 1 for count, name, spot, _ in g if name == "last")
    assert not any(int(r[3]) == 0 for r in runs(cases, "carry"))


def test_evaluation_cases(cases):
    f = cases.facts["eval"]
    assert [(d["n"], d["slices"]) for d in f] == [(256, 1), (512, 1), (1024, 1), (4096, 16), (8192, 16), (65536, 16)]
    for d in f:
        n, jobs = d["n"], d["jobs"]
        assert len(d["bw"]) == 6 and all(0 <= r < 6 for _, rots in jobs for r in rots)
        assert any(len(set(rots)) < len(rots) for _, rots in jobs)                         # a repeated rotation
        assert len({id(col) for col, _ in jobs}) < len(jobs)                              # two jobs share a column
        assert any(set(col) == {R - 1} and set(d["bw"][rots[0]]) == {R - 1} for col, rots in jobs)
        singles = {col.index(R - 1) for col, _ in jobs if col.count(0) == n - 1}
        if n < 65536:
            assert {len(rots) for _, rots in jobs} == {1, 2, 3, 4} and any(not any(col) for col, _ in jobs)
            assert singles == {0, 255, 256 % n, n - 1}
        else:
            assert singles == {n - 1}
        assert SENT in d["out"]   # an unused slot to find untouched


def test_lincomb_cases(cases):
    f = cases.facts["lincomb"]
    assert sorted({(d["m"], d["per"]) for d in f}) == [(1, 0), (2, 0), (47, 0), (48, 0), (49, 48), (96, 48), (97, 48)]
    for d in f:
        sizes = [hi - lo for lo, hi in d["bounds"]]
        assert sizes == {1: [1], 2: [2], 47: [47], 48: [48], 49: [48, 1], 96: [48, 48], 97: [48, 48, 1]}[d["m"]]
        if d["name"] == "mixed":
            assert 0 in d["s29"] and (d["m"] < 6 or len(set(d["which"])) < d["m"])
        else:
            assert set(d["s29"]) == {R - 1} and set(d["which"]) == {1}
    assert {int(r[3]) for r in runs(cases, "lincomb")} == {1, 2}


def test_quotient_combine_and_shplonk_cases(cases):
    q = cases.facts["qcombine"]
    assert {(rows, ng) for rows, ng, _, _, _ in q} == {(rows, ng) for rows in (3, 4) for ng in (1, 2, 7, 8)}
    assert {(pt0, cnt == rows * 512) for rows, _, _, pt0, cnt in q} == {(0, True), (512, False)}
    s = cases.facts["shplonk"]
    assert [d["ns"] for d in s] == [1, 5, 8]
    for d in s:
        assert all(1 <= x["n_pts"] <= 4 and not any(x["rc"][x["n_pts"]:]) for x in d["sets"])
        assert [i for row in d["zs"] for i, x in enumerate(row) if x == 0] == [37]
    assert {x["n_pts"] for d in s for x in d["sets"]} == {1, 2, 3, 4}
    assert cases.facts["bary_den"].count(0) == 2


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_compiles_for_gfx950(tmp_path):
    """compile only: the device pass for gfx950 with the library's flags, no link, nothing run"""
    from zk_fhe_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    t0 = time.time()
    subprocess.run([hipcc, *build.FLAGS, "-I", os.path.join(ROOT, "zk-fhe_amd", "host"), "-I", build.CSRC, "-c",
                    os.path.join(HERE, "native", "prover_kernels_driver.hip"), "-o", str(tmp_path / "driver.o")], check=True)
    print("prover_kernels_driver: compiled in %.1f s" % (time.time() - t0))
