"""The case list of tests/native/prover_kernels_driver.hip and what every case has to give, in Python integers only.

Conventions, used everywhere below:
  * a word in memory is x 2^256 mod r, canonical: `W(x)`;
  * `a * b` in a kernel is a b 2^-256 mod r on words: `mulw(a, b)`;
  * a constant in the "2^261 form" is a canonical word w, and fr29_mul(v, w) = v w 2^-261 mod r (zk-fhe_amd/csrc/fr29.hip.hpp,
    lines 1-7): `mul29(v, w)`;
  * the edge words are WORDS of tests/test_gpu_fr_edges.py and GRID of tests/test_gpu_fr9_kernels.py;
  * a buffer the driver does not load starts as bytes 0xA5: `SENT` is a word of them, no canonical value.

`build()` returns the text of cases.txt, the input files and the checks: per group a list of (case, buffer, expected bytes, mask) --
the words of the buffer where mask is true (all, if None) must equal the expected ones.  tests/test_prover_kernels_host.py checks the
reference functions against other statements of the same operations, and that the list holds the edges it is meant to hold."""
import functools
import random

import numpy as np

from oracle import halo2_ref as H
from oracle import pyref
from tests.test_gpu_fr9_kernels import GRID
from tests.test_gpu_fr_edges import WORDS

R = pyref.R
MONT = 1 << 256
RINV = pow(MONT, -1, R)
RINV261 = pow(1 << 261, -1, R)
ONE = MONT % R                      # the word of 1
SENT = int.from_bytes(b"\xa5" * 32, "little")
EDGE = sorted(set(WORDS) | set(GRID))
M = len(EDGE)
N = 512
OMEGA9 = pyref.root_of_unity(9)


def W(x):
    return x * MONT % R


def mulw(a, b):
    return a * b * RINV % R


def mul29(v, w):
    return v * w * RINV261 % R


def invw(a):
    """the word of 1 / x for the word a of x; zero stays zero"""
    return pow(a, R - 2, R) * MONT * MONT % R


def to_bytes(words):
    return b"".join(int(x).to_bytes(32, "little") for x in words)


def hexw(x):
    return "%064x" % x


def wpow_words(log_n):
    w, out, x = pyref.root_of_unity(log_n), [], 1
    for _ in range(1 << log_n):
        out.append(W(x))
        x = x * w % R
    return out


def edge_cycle(n, stride, start):
    return [EDGE[(start + i * stride) % M] for i in range(n)]


# ------------------------------------------------------------------------------------------------ references
def ref_prefix(ratio, u):
    """z[0] = 1, z[i + 1] = z[i] ratio[i] for i < u: u + 1 words"""
    z = [ONE]
    for i in range(u):
        z.append(mulw(z[-1], ratio[i]))
    return z


def ref_eval(col, w, lo=0, hi=None):
    """sum_i col[i] w[i] 2^-261 over rows [lo, hi)"""
    hi = len(col) if hi is None else hi
    return sum(col[i] * w[i] for i in range(lo, hi)) * RINV261 % R


def ref_lincomb(cols, s29, i):
    return sum(c[i] * s for c, s in zip(cols, s29)) * RINV261 % R


def ref_sh_zs(pts, w):
    acc = ONE
    for p in pts:
        acc = mulw(acc, (w - p) % R)
    return acc


def ref_sh_h(sets, F, zs_inv, wpow):
    """sets: dicts with rc (4 words), vj; hq[i] = sum_j vj (F_j[i] - r_j(w^i)) zs_inv[j][i]"""
    out = []
    for i, w in enumerate(wpow):
        acc = 0
        for j, s in enumerate(sets):
            r = s["rc"][3]
            for k in (2, 1, 0):
                r = (mulw(r, w) + s["rc"][k]) % R
            acc += mulw(mulw(s["vj"], (F[j][i] - r) % R), zs_inv[j][i])
        out.append(acc % R)
    return out


def ref_sh_w(coef, r_u, F, hq, ztu, inv):
    out = []
    for i in range(len(hq)):
        acc = sum(mulw(coef[j], (F[j][i] - r_u[j]) % R) for j in range(len(F)))
        out.append(mulw((acc - mulw(ztu, hq[i])) % R, inv[i]))
    return out


def rng_row_words(seed, first, count):
    """draws first .. first + count - 1 of oracle/halo2_ref.py's Rng, as words"""
    g = H.Rng(seed)
    g.ctr = first
    return [W(g.next()) for _ in range(count)]


# ------------------------------------------------------------------------------------------------ the list
class Cases:
    def __init__(self):
        self.lines = []
        self.files = {}      # input file -> bytes
        self.checks = {}     # group -> [(case, buffer, expected bytes, mask)]
        self.facts = {}      # what the host test asserts about the list itself
        self._n = 0

    def text(self):
        return "\n".join(self.lines) + "\n"

    def load(self, words, raw=None):
        """a buffer holding these words (or raw bytes); returns its name"""
        self._n += 1
        name = "b%d" % self._n
        data = to_bytes(words) if raw is None else raw
        self.files[name + ".bin"] = data
        self.lines.append("buf %s %d %s.bin" % (name, len(data), name))
        return name

    def out(self, n_words=0, n_bytes=None):
        """a buffer of sentinel bytes"""
        self._n += 1
        name = "b%d" % self._n
        self.lines.append("buf %s %d -" % (name, n_words * 32 if n_bytes is None else n_bytes))
        return name

    def run(self, case, kernel, *args):
        self.lines.append("run %s %s %s" % (case, kernel, " ".join(str(a) for a in args)))

    def expect(self, group, case, buf, words, mask=None, raw=None):
        if not any(l == "dump " + buf for l in self.lines[-40:]):
            self.lines.append("dump " + buf)
        self.checks.setdefault(group, []).append((case, buf, to_bytes(words) if raw is None else raw, mask))


def blocks(work):
    """grid_for's shape: ceil(work / 256) workgroups; its cap of 16 per compute unit is far away at these sizes"""
    b = -(-work // 256)
    assert 1 <= b <= 64
    return b


def grids(work):
    """the prover's grid and two workgroups; one where two would still give every element a thread of its own"""
    return sorted({blocks(work), 2} | ({1} if work <= 512 else set()))


def perm_cases(c, rnd):
    n, n_adv, n_perm = N, 5, 7
    wpow = wpow_words(9)
    beta, gamma = rnd.randrange(R), rnd.randrange(R)
    bd = [beta]
    for _ in range(n_perm - 1):
        bd.append(mulw(bd[-1], W(pyref.FR_DELTA)))
    cols = [edge_cycle(n, 1, 0), [rnd.randrange(R) for _ in range(n)], edge_cycle(n, 5, 3), [rnd.randrange(R) for _ in range(n)], edge_cycle(n, 7, 11),
            edge_cycle(n, 3, 2), [rnd.randrange(R) if i < 40 else 0 for i in range(n)]]   # five advice columns, the constants, the instance
    sigma = [[rnd.randrange(R) for _ in range(n)] if k % 2 else edge_cycle(n, 2 * k + 1, k) for k in range(n_perm)]
    # planted zeros: (column, row) of a zero factor of the numerator / of the denominator
    num_zero, den_zero = [(5, 17), (1, 511)], [(6, 300), (3, 0)]
    for k, i in num_zero:
        cols[k][i] = -(mulw(bd[k], wpow[i]) + gamma) % R
    for k, i in den_zero:
        cols[k][i] = -(mulw(beta, sigma[k][i]) + gamma) % R
    c.facts["perm"] = dict(num_zero=num_zero, den_zero=den_zero, n_perm=n_perm, n_adv=n_adv)
    adv = c.load([x for col in cols[:n_adv] for x in col])
    const, inst = c.load(cols[5]), c.load(cols[6])
    sig, wp, bdb = c.load([x for col in sigma for x in col]), c.load(wpow), c.load(bd)
    nf = [[(cols[k][i] + mulw(bd[k], wpow[i]) + gamma) % R for i in range(n)] for k in range(n_perm)]
    df = [[(cols[k][i] + mulw(beta, sigma[k][i]) + gamma) % R for i in range(n)] for k in range(n_perm)]
    for chunk in (3, 7, 1):
        nch = -(-n_perm // chunk)
        num, den = [], []
        for j in range(nch):
            members = range(j * chunk, min((j + 1) * chunk, n_perm))
            for i in range(n):
                a = b = ONE
                for k in members:
                    a, b = mulw(a, nf[k][i]), mulw(b, df[k][i])
                num.append(a)
                den.append(b)
        c.facts["perm"]["chunk%d" % chunk] = (num, den)
        for grid in grids(nch * n):
            case = "perm_chunk%d_grid%d" % (chunk, grid)
            o_num, o_den = c.out(nch * n), c.out(nch * n)
            c.run(case, "perm", grid, n, n_adv, n_perm, chunk, adv, const, inst, sig, wp, bdb, hexw(beta), hexw(gamma), o_num, o_den)
            c.expect("perm", case, o_num, num)
            c.expect("perm", case, o_den, den)


def lookup_cases(c, rnd):
    n = N
    c.facts["lookup"] = []
    for name, beta, gamma in (("random", rnd.randrange(R), rnd.randrange(R)), ("rm1", R - 1, R - 1), ("zero", 0, 0)):
        for nl in (1, 3):
            a = [[rnd.randrange(R) for _ in range(n)] for _ in range(nl)]
            la = [edge_cycle(n, 3, l) for l in range(nl)]
            ls = [[rnd.randrange(R) for _ in range(n)] for _ in range(nl)]
            table = edge_cycle(n, 1, 5)
            for l in range(nl):
                a[l][3 + l] = -beta % R                  # a + beta = 0
                la[l][9 + l] = -beta % R                 # a' + beta = 0
                ls[l][100 + l] = -gamma % R              # s' + gamma = 0
                for i, v in enumerate((0, 255, R - 1, W(255), W(R - 1))):
                    a[l][20 + i], la[l][30 + i], ls[l][40 + i] = v, v, v
            table[200] = -gamma % R                      # s + gamma = 0
            table[50:55] = [0, 255, R - 1, W(255), W(R - 1)]
            num = [mulw((a[l][i] + beta) % R, (table[i] + gamma) % R) for l in range(nl) for i in range(n)]
            den = [mulw((la[l][i] + beta) % R, (ls[l][i] + gamma) % R) for l in range(nl) for i in range(n)]
            c.facts["lookup"].append(dict(beta=beta, gamma=gamma, a=a, la=la, ls=ls, table=table, num=num, den=den, nl=nl))
            ab, tb, lab, lsb = c.load([x for col in a for x in col]), c.load(table), c.load([x for col in la for x in col]), c.load([x for col in ls for x in col])
            for grid in grids(nl * n):
                case = "lookup_%s_nl%d_grid%d" % (name, nl, grid)
                o_num, o_den = c.out(nl * n), c.out(nl * n)
                c.run(case, "lookup", grid, n, nl, ab, tb, lab, lsb, hexw(beta), hexw(gamma), o_num, o_den)
                c.expect("lookup", case, o_num, num)
                c.expect("lookup", case, o_den, den)


def z_bytes(z, n):
    """a column of z: the defined rows, sentinel words above"""
    return to_bytes(z) + b"\xa5" * (32 * (n - len(z)))


def prefix_columns(rnd, n, boundary):
    """the columns that do not depend on u: random, all ones, all r - 1 (the value -1: products alternate), a single zero at row 0
    and one at `boundary`; their running products over all n rows"""
    rand = [rnd.randrange(1, R) for _ in range(n)]
    z0, zb = list(rand), list(rand)
    z0[0] = 0
    zb[boundary] = 0
    cols = dict(random=rand, ones=[ONE] * n, minus_one=[W(R - 1)] * n, zero_row0=z0, zero_boundary=zb)
    zfull = {k: ref_prefix(v, n - 1) for k, v in cols.items()}
    return cols, zfull


def u_columns(rand, zrand, u):
    """the columns that depend on u, cut from the random one: a zero at row u - 1 (z[u] alone is zero), and a last ratio that makes the
    product exactly 1"""
    zl, p1 = list(rand), list(rand)
    zl[u - 1] = 0
    p1[u - 1] = invw(zrand[u - 1])
    return dict(zero_last=(zl, zrand[:u] + [0]), product_one=(p1, zrand[:u] + [ONE]))


NO_BLIND = (0, 0, 0, 0, 0, 0, 0)


def prefix_cases(c, rnd):
    c.facts["prefix"] = []
    for n, m in ((512, 384), (1024, 640), (2048, 1022), (65536, 44800)):
        per = -(-n // 1024)
        assert m % per == 0
        boundary = per * 100
        cols, zfull = prefix_columns(rnd, n, boundary)
        names = list(cols)
        shared = c.load([x for k in names for x in cols[k]])
        for u in (n - 7 if n == 512 else n - 107, n - 1, m - 1, m, m + 1):
            case = "prefix_n%d_u%d" % (n, u)
            z, tot = c.out(len(names) * n), c.out(len(names))
            c.run(case, "prefix", n, u, len(names), shared, z, tot, *NO_BLIND)
            c.expect("prefix", case, z, None, raw=b"".join(z_bytes(zfull[k][:u + 1], n) for k in names))
            c.expect("prefix", case, tot, [zfull[k][u] for k in names])
            ucols = u_columns(cols["random"], zfull["random"], u)
            inp = c.load([x for k in ucols for x in ucols[k][0]])
            z, tot = c.out(2 * n), c.out(2)
            c.run(case + "_u", "prefix", n, u, 2, inp, z, tot, *NO_BLIND)
            c.expect("prefix", case + "_u", z, None, raw=b"".join(z_bytes(ucols[k][1], n) for k in ucols))
            c.expect("prefix", case + "_u", tot, [ucols[k][1][u] for k in ucols])
            c.facts["prefix"].append(dict(n=n, u=u, per=per, boundary=boundary, cols=cols, zfull=zfull, ucols=ucols))
    # blinding rows drawn by the workgroups behind the columns'
    n, u, seed, ctr0, stride = 1024, 1024 - 107, bytes(range(7, 39)), 1000, 5000
    cols = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(3)]
    exp = b"".join(to_bytes(ref_prefix(cols[k], u) + rng_row_words(seed, ctr0 + k * stride, n - u - 1)) for k in range(3))
    inp, z, tot = c.load([x for col in cols for x in col]), c.out(3 * n), c.out(3)
    c.run("prefix_blind", "prefix", n, u, 3, inp, z, tot, 1, *[int.from_bytes(seed[8 * i:8 * i + 8], "little") for i in range(4)], ctr0, stride)
    c.expect("prefix", "prefix_blind", z, None, raw=exp)
    c.expect("prefix", "prefix_blind", tot, [ref_prefix(cols[k], u)[u] for k in range(3)])
    c.facts["prefix_blind"] = dict(n=n, u=u, ctr0=ctr0, stride=stride)


def prefix_seg_cases(c, rnd):
    """every input goes through the three segment kernels and through k_prefix_product: both have to give the same words"""
    n, seg_len = 1 << 17, 32768
    cols, zfull = prefix_columns(rnd, n, 2 * seg_len)   # the zero on a segment boundary
    cols["zero_seg0"] = list(cols["random"])
    cols["zero_seg0"][5] = 0
    zfull["zero_seg0"] = zfull["random"][:6] + [0] * (n - 6)
    del cols["zero_row0"], zfull["zero_row0"]
    cols["random2"] = [rnd.randrange(1, R) for _ in range(n)]
    zfull["random2"] = ref_prefix(cols["random2"], n - 1)
    names = list(cols)
    assert len(names) == 6
    shared = c.load([x for k in names for x in cols[k]])
    c.facts["prefix_seg"] = []
    for u in (n - 107, n - 1, 3 * seg_len):
        pairs = [(shared + "+%d" % (32 * n * p), [zfull[k][:u + 1] for k in names[p:p + 2]]) for p in (0, 2, 4)]
        ucols = u_columns(cols["random"], zfull["random"], u)   # u - 1 lies in the last segment, or is the last row of the one before
        pairs.append((c.load([x for k in ucols for x in ucols[k][0]]), [ucols[k][1] for k in ucols]))
        c.facts["prefix_seg"].append(dict(n=n, u=u, seg_len=seg_len, cols=cols, ucols=ucols))
        for p, (inp, zs) in enumerate(pairs):
            exp_z, exp_tot = b"".join(z_bytes(z, n) for z in zs), [z[u] for z in zs]
            case = "prefix_seg_u%d_pair%d" % (u, p)
            seg, z, tot = c.out(2 * 4), c.out(2 * n), c.out(2)
            c.run(case, "prefix_seg", n, u, 2, seg_len, inp, seg, z, tot)
            c.expect("prefix_seg", case, z, None, raw=exp_z)
            c.expect("prefix_seg", case, tot, exp_tot)
            z, tot = c.out(2 * n), c.out(2)
            c.run(case + "_one_workgroup", "prefix", n, u, 2, inp, z, tot, *NO_BLIND)
            c.expect("prefix_seg", case + "_one_workgroup", z, None, raw=exp_z)
            c.expect("prefix_seg", case + "_one_workgroup", tot, exp_tot)


CARRY_COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, 4096)
TAIL = [SENT, SENT, SENT]   # words behind the totals, part of the loaded array: they must come back as they were


def carry_cases(c, rnd):
    c.facts["carry"] = []
    for count in CARRY_COUNTS:
        tot = [rnd.randrange(1, R) for _ in range(count)]
        p = ONE
        for t in tot[:-1]:
            p = mulw(p, t)
        tot[-1] = invw(p)   # the product of all is exactly 1
        doubled = tot[:-1] + [tot[-1] * 2 % R]
        zero = list(tot)
        zero[count // 2] = 0
        for name, totals, closes in (("closes", tot, 1), ("doubled", doubled, 0), ("zero", zero, 0)):
            case = "carry_%d_%s" % (count, name)
            carry = ref_prefix(totals, count)
            assert (carry[count] == ONE) == bool(closes)
            b, flag = c.load(totals + TAIL), c.out(n_bytes=4)
            c.run(case, "carry", count, 0, b, flag)
            c.expect("carry", case, b, carry[:count] + TAIL)
            c.expect("carry", case, flag, None, raw=closes.to_bytes(4, "little"))
            c.facts["carry"].append((count, name, totals))


def carry_ones_cases(c, rnd):
    c.facts["carry_ones"] = []
    for count in (1, 3, 1024, 1025, 4096):
        per = -(-count // 1024)
        spots = {"all_ones": None, "first": 0, "last": count - 1}
        if per > 1:
            spots["second_slot"] = per * 1 + 1   # thread 1's second total
        for name, spot in spots.items():
            totals = [ONE] * count + [W(2), SENT, SENT]   # a canonical word that is not one just behind the totals
            if spot is not None:
                totals[spot] = W(2) if spot else ONE + 1
            closes = 1 if spot is None else 0
            case = "carry_ones_%d_%s" % (count, name)
            b, flag = c.load(totals), c.out(n_bytes=4)
            c.run(case, "carry", count, 1, b, flag)
            c.expect("carry_ones", case, b, totals)
            c.expect("carry_ones", case, flag, None, raw=closes.to_bytes(4, "little"))
            c.facts["carry_ones"].append((count, name, spot, per))


def scale_cases(c, rnd):
    n, u, n_cols = N, N - 7, 3
    z = [edge_cycle(n, 1, 4), [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]]
    carry = [R - 1, rnd.randrange(R), ONE]
    exp = [mulw(z[k][i], carry[k]) if i <= u else z[k][i] for k in range(n_cols) for i in range(n)]
    cb = c.load(carry)
    for grid in (blocks(n_cols * (u + 1)), 2):
        case = "scale_grid%d" % grid
        zb = c.load([x for col in z for x in col])
        c.run(case, "scale", grid, n, u + 1, n_cols, zb, cb)
        c.expect("scale", case, zb, exp)


def eval_cases(c, rnd):
    c.facts["eval"] = []
    for n, slices in ((256, 1), (512, 1), (1024, 1), (4096, 16), (8192, 16), (65536, 16)):
        bw = [[rnd.randrange(R) for _ in range(n)], [R - 1] * n, [rnd.randrange(R) for _ in range(n)], edge_cycle(n, 1, 0),
              [rnd.randrange(R) for _ in range(n)], edge_cycle(n, 5, 7)]
        rand, rand2 = [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]

        def single(row):
            col = [0] * n
            col[row] = R - 1
            return col
        # (column, rotation indices in use); every job's unused indices are 0
        if n < 65536:
            jobs = [(rand, [0]), (rand, [1, 2]), (rand2, [3, 4, 5]), (rand2, [0, 1, 2, 3]), ([R - 1] * n, [1, 1, 0, 1]), ([0] * n, [0, 1])]
            jobs += [(single(row), [2, 1]) for row in sorted({0, 255, 256 % n, n - 1})]
        else:
            jobs = [(rand, [0]), (rand, [0, 1, 2, 3]), ([R - 1] * n, [1, 1, 0, 1]), (single(n - 1), [2])]
        col_bufs = {}
        for col, _ in jobs:
            if id(col) not in col_bufs:
                col_bufs[id(col)] = c.load(col)
        nj = len(jobs)
        step = n // slices
        partial = [SENT] * (slices * nj * 4)
        out = [SENT] * (nj * 4)
        args = []
        for j, (col, rots) in enumerate(jobs):
            for r, rot in enumerate(rots):
                parts = [ref_eval(col, bw[rot], y * step, (y + 1) * step) for y in range(slices)]
                for y in range(slices):
                    partial[(y * nj + j) * 4 + r] = parts[y]
                out[j * 4 + r] = sum(parts) % R
            args += [col_bufs[id(col)], len(rots)] + (rots + [0, 0, 0])[:4]
        bwb, pb, ob = c.load([x for row in bw for x in row]), c.out(slices * nj * 4), c.out(nj * 4)
        case = "eval_n%d" % n
        c.run(case, "eval", n, slices, blocks(nj * 4), nj, bwb, pb, ob, *args)
        if slices == 1:
            c.expect("eval", case, ob, out)
            c.expect("eval", case, pb, [SENT] * (nj * 4))   # the single-slice launch does not touch the buffer of the slices
        else:
            c.expect("eval", case, pb, partial)
            c.expect("eval", case, ob, out, mask=np.array([w != SENT for w in out]))   # k_sum_rows adds the unused slots' sentinels up: not compared
        c.facts["eval"].append(dict(n=n, slices=slices, jobs=jobs, bw=bw, out=out))


def lincomb_cases(c, rnd):
    n = N
    pool = [[rnd.randrange(R) for _ in range(n)], [R - 1] * n, edge_cycle(n, 1, 0), [rnd.randrange(R) for _ in range(n)], [0] * n, edge_cycle(n, 7, 3)]
    pb = c.load([x for col in pool for x in col])
    c.facts["lincomb"] = []
    for m, per in ((1, 0), (2, 0), (47, 0), (48, 0), (49, 48), (96, 48), (97, 48)):
        for name in ("mixed", "rm1"):
            if name == "mixed":
                which = [(3 * k + k // 6) % 6 for k in range(m)]   # several pointers to the same column
                s29 = [rnd.randrange(R) if k % 3 else EDGE[k % M] for k in range(m)]
                s29[m // 2] = 0
                if m > 2:
                    s29[0], which[0] = R - 1, 1
            else:
                which, s29 = [1] * m, [R - 1] * m   # every term (r - 1)^2: the lazy sum as high as it gets
            cols = [pool[w] for w in which]
            chunks = -(-m // per) if per else 1
            bounds = [(k * per, min((k + 1) * per, m)) for k in range(chunks)] if per else [(0, m)]
            partial = [ref_lincomb(cols[lo:hi], s29[lo:hi], i) for lo, hi in bounds for i in range(n)]
            out = [sum(partial[k * n + i] for k in range(chunks)) % R for i in range(n)]
            sb = c.load(s29)
            c.facts["lincomb"].append(dict(m=m, per=per, name=name, which=which, s29=s29, bounds=bounds))
            for grid in (blocks(n), 1):   # the prover's two workgroups, and one: every thread strides
                case = "lincomb_m%d_%s_grid%d" % (m, name, grid)
                part_b, ob = c.out(chunks * n), c.out(n)
                c.run(case, "lincomb", grid, n, per, m, part_b, ob, sb, *["%s+%d" % (pb, 32 * n * w) for w in which])
                c.expect("lincomb", case, ob, out)
                c.expect("lincomb", case, part_b, partial if per else [SENT] * n)


def qcombine_cases(c, rnd):
    log_n, n = 9, N
    c.facts["qcombine"] = []
    for rows in (3, 4):
        ne = rows * n
        for ng in (1, 2, 7, 8):
            for name in ("mixed", "rm1"):
                if name == "mixed":
                    partials = [edge_cycle(ne, g + 1, g) if g % 2 == 0 else [rnd.randrange(R) for _ in range(ne)] for g in range(ng)]
                    ypow = [EDGE[(5 * g + 4) % M] if g % 3 else rnd.randrange(R) for g in range(ng)]
                    zinv = [R - 1, rnd.randrange(R), EDGE[7], rnd.randrange(R)][:rows]
                else:
                    partials, ypow, zinv = [[R - 1] * ne] * ng, [R - 1] * ng, [R - 1] * rows
                h = [mul29(sum(mul29(partials[g][p], ypow[g]) for g in range(ng)) % R, zinv[p >> log_n]) for p in range(ne)]
                pb, yb, zb = c.load([x for row in partials for x in row]), c.load(ypow), c.load(zinv)
                for pt0, cnt in ((0, ne), (n, n)):
                    case = "qcombine_rows%d_g%d_%s_pt%d" % (rows, ng, name, pt0)
                    ob = c.out(ne)
                    c.run(case, "qcombine", log_n, rows, ng, pt0, cnt, pb, yb, zb, ob)
                    c.expect("qcombine", case, ob, [h[p] if pt0 <= p < pt0 + cnt else SENT for p in range(ne)])
                    c.facts["qcombine"].append((rows, ng, name, pt0, cnt))


def small_cases(c, rnd):
    n = N
    wpow = wpow_words(9)
    wp = c.load(wpow)
    for name in ("mixed", "rm1"):
        if name == "mixed":
            rows3 = [x for k in range(3) for x in (edge_cycle(n, k + 1, k) if k != 1 else [rnd.randrange(R) for _ in range(n)])]
            pw = [x for k in range(3) for x in (edge_cycle(n, 3, 2 * k) if k == 1 else [rnd.randrange(R) for _ in range(n)])]
            vinv = [EDGE[(4 * k + 1) % M] if k % 2 else rnd.randrange(R) for k in range(9)]
        else:
            rows3, pw, vinv = [R - 1] * (3 * n), [R - 1] * (3 * n), [R - 1] * 9
        t = [mulw(a, b) for a, b in zip(rows3, pw)]
        h_c = [sum(mulw(vinv[3 * m + k], t[k * n + i]) for k in range(3)) % R for m in range(3) for i in range(n)] + [0] * n
        rb, pwb, ob = c.load(rows3), c.load(pw), c.out(4 * n)
        c.run("ext3_" + name, "ext3", n, rb, pwb, ob, *[hexw(v) for v in vinv])
        c.expect("small", "ext3_" + name, ob, h_c)
    pts = [0, R - 1, wpow[77], rnd.randrange(R), ONE, EDGE[9]]   # wpow[0] is the word of 1: two of the points lie on the domain
    den = [(p - w) % R for p in pts for w in wpow]
    c.facts["bary_den"] = den
    ptb = c.load(pts)
    for grid in (blocks(6 * n), 2):
        ob = c.out(6 * n)
        c.run("bary_den_grid%d" % grid, "bary_den", grid, n, 6, wp, ptb, ob)
        c.expect("small", "bary_den_grid%d" % grid, ob, den)
    for cc in (R - 1, rnd.randrange(R)):
        inv = [x for k in range(6) for x in (edge_cycle(n, k + 1, k) if k % 2 else [rnd.randrange(R) for _ in range(n)])]
        want = [mulw(mulw(x, wpow[g % n]), cc) for g, x in enumerate(inv)]
        for grid in (blocks(6 * n), 2):
            case = "bary_weights_%s_grid%d" % ("rm1" if cc == R - 1 else "random", grid)
            b = c.load(inv)
            c.run(case, "bary_weights", grid, n, 6 * n, wp, hexw(cc), b)
            c.expect("small", case, b, want)
    values = [0, ONE, R - 1, W(R - 1), rnd.randrange(R)]
    for n_pow in (1, 7, 300):
        for si, start in enumerate(values):
            for bi, base in enumerate(values):
                sv, bv = start * RINV % R, base * RINV % R
                want = [W(sv * pow(bv, i, R)) for i in range(n_pow)]
                for grid in sorted({1, blocks(n_pow)}):   # one workgroup (the prover's launch of a short table: 300 strides) and ceil(n / 256)
                    case = "powers_n%d_s%d_b%d_grid%d" % (n_pow, si, bi, grid)
                    ob = c.out(n_pow + 1)
                    c.run(case, "powers", grid, n_pow, hexw(start), hexw(base), ob)
                    c.expect("small", case, ob, want + [SENT])


def shset_bytes(s):
    return to_bytes(s["rc"] + s["pts"] + [s["vj"], s["coef"], s["r_u"]]) + np.array([s["n_pts"], 0, 0, 0], dtype="<i4").tobytes()


def shplonk_cases(c, rnd):
    n = N
    wpow = wpow_words(9)
    wp = c.load(wpow)
    c.facts["shplonk"] = []
    for ns in (1, 5, 8):
        sets = []
        for j in range(ns):
            n_pts = 1 + (j + ns) % 4   # 1 .. 4 among the sets; a single set has two points
            pts = [rnd.randrange(R) for _ in range(n_pts)]
            if j == ns - 1:
                pts[0] = wpow[37]      # a point on the domain: zs has a zero at row 37
            sets.append(dict(n_pts=n_pts, pts=pts + [0] * (4 - n_pts), rc=[EDGE[(3 * j + k) % M] if k % 2 else rnd.randrange(R) for k in range(n_pts)] + [0] * (4 - n_pts),
                             vj=EDGE[(j + 3) % M] if j % 2 else rnd.randrange(R), coef=EDGE[(2 * j + 4) % M] if j != 2 else rnd.randrange(R),
                             r_u=EDGE[(5 * j + 1) % M] if j % 2 == 0 else rnd.randrange(R)))
        F = [edge_cycle(n, j + 1, j) if j % 3 == 1 else [rnd.randrange(R) for _ in range(n)] for j in range(ns)]
        zs = [[ref_sh_zs(s["pts"][:s["n_pts"]], w) for w in wpow] for s in sets]
        zs_inv = [[invw(x) for x in row] for row in zs]   # the zero stays a zero: it is never inverted
        hq = ref_sh_h(sets, F, zs_inv, wpow)
        inv = [rnd.randrange(R) if i % 4 else EDGE[i % M] for i in range(n)]
        c.facts["shplonk"].append(dict(ns=ns, sets=sets, zs=zs))
        sb, Fb, zib, hqb, invb = c.load(None, raw=b"".join(shset_bytes(s) for s in sets)), c.load([x for row in F for x in row]), c.load([x for row in zs_inv for x in row]), c.load(hq), c.load(inv)
        for grid in sorted({blocks(ns * n), 2}):
            ob = c.out(ns * n)
            c.run("sh_zs_%d_grid%d" % (ns, grid), "sh_zs", grid, n, ns, sb, wp, ob)
            c.expect("shplonk", "sh_zs_%d_grid%d" % (ns, grid), ob, [x for row in zs for x in row])
        coef, r_u = [s["coef"] for s in sets] + [R - 1] * (8 - ns), [s["r_u"] for s in sets] + [R - 2] * (8 - ns)   # the slots past n_sets hold words the kernel must not use
        for grid in (blocks(n), 1):   # the prover's two workgroups, and one: every thread strides
            ob = c.out(n)
            c.run("sh_h_%d_grid%d" % (ns, grid), "sh_h", grid, n, ns, sb, Fb, zib, wp, ob)
            c.expect("shplonk", "sh_h_%d_grid%d" % (ns, grid), ob, hq)
            for ztu in (R - 1, EDGE[6], rnd.randrange(R)):
                case = "sh_w_%d_grid%d_ztu%x" % (ns, grid, ztu & 0xFFFF)
                ob = c.out(n)
                c.run(case, "sh_w", grid, n, ns, Fb, hqb, invb, ob, hexw(ztu), *[hexw(x) for x in coef + r_u])
                c.expect("shplonk", case, ob, ref_sh_w(coef[:ns], r_u[:ns], F, hq, ztu, inv))
    for name, u in (("on_domain", wpow[5]), ("rm1", R - 1), ("zero", 0), ("random", rnd.randrange(R))):
        ob = c.out(n)
        c.run("sh_den_" + name, "sh_den", n, wp, hexw(u), ob)
        c.expect("shplonk", "sh_den_" + name, ob, [(w - u) % R for w in wpow])


GROUPS = ("perm", "lookup", "prefix", "prefix_seg", "carry", "carry_ones", "scale", "eval", "lincomb", "qcombine", "small", "shplonk")


@functools.lru_cache(maxsize=None)
def build():
    c = Cases()
    for k, f in enumerate((perm_cases, lookup_cases, prefix_cases, prefix_seg_cases, carry_cases, carry_ones_cases, scale_cases, eval_cases, lincomb_cases,
                           qcombine_cases, small_cases, shplonk_cases)):
        f(c, random.Random(1000 + k))
    assert set(c.checks) == set(GROUPS)
    return c


def mismatches(c, group, read):
    """read(buffer) -> the bytes the driver wrote; returns a list of '<case> <buffer>: first differing word' lines"""
    bad = []
    for case, buf, want, mask in c.checks[group]:
        got = read(buf)
        if len(got) != len(want):
            bad.append("%s %s: %d bytes, expected %d" % (case, buf, len(got), len(want)))
            continue
        if len(want) % 32:
            if got != want:
                bad.append("%s %s: %r, expected %r" % (case, buf, got, want))
            continue
        g, w = np.frombuffer(got, dtype=np.uint64).reshape(-1, 4), np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
        diff = (g != w).any(axis=1)
        if mask is not None:
            diff &= mask
        if diff.any():
            i = int(np.argmax(diff))
            bad.append("%s %s: %d words differ, the first at %d: %064x, expected %064x" % (case, buf, int(diff.sum()), i, int.from_bytes(g[i].tobytes(), "little"),
                                                                                           int.from_bytes(w[i].tobytes(), "little")))
    return bad
