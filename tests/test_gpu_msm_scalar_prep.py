"""What k_msm_table does with a scalar before any point is added (csrc/msm_table.hip.hpp): out of Montgomery form through the
nine-limb reduction, sign split, bias, and the signed digits of the table's windows -- at a literal width (k_msm_table<TREE, C>,
C = 9, 11, 13, 15) or at a run-time one (C = 0: every other width, and every width under ZKFHE_TABLE_GENERIC=1).

Smallest geometry that gets a table (n = 256; n = 300 for a partial last chunk), the scalars at which a digit, a carry or the sign
flips, on 1 column (TREE, one partial per visit), 3 columns and 17 (the smallest call with TREE = false: msm_table's
`tree = n_cols <= 16`).  Against the oracle MSM (oracle/oracle.c orc_msm, the reference of tests/test_gpu_parity.py), bit for bit;
and the launcher's count of mixed additions against the number of non-zero signed digits worked out here in Python integers: the
same additions as before, only cheaper to find."""
import os

import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref

pytestmark = pytest.mark.gpu
R = pyref.R
HALF_R = (R - 1) // 2
SPECIALISED = (9, 11, 13, 15)
GENERIC = 10                    # a width without an instantiation of its own
N_COLS = (1, 3, 17)             # TREE with one column, TREE with a few, the smallest call without (n_cols > 16)
N_FULL, N_PART = 256, 300       # one whole 256-chunk (two of 128); 300: the last chunk is partial whether P is 128 or 256


def windows(c):
    return (255 + c - 1) // c


def signed_digits(s, c):
    """the biasing rule of csrc/msm_table.hip.hpp in integers: |s| + sum_w 2^(c w + c - 1), window w minus 2^(c - 1)"""
    m = R - s if s > HALF_R else s
    t = m + sum(1 << (c * w + c - 1) for w in range(windows(c)))
    d = [((t >> (c * w)) & ((1 << c) - 1)) - (1 << (c - 1)) for w in range(windows(c))]
    assert sum(x << (c * w) for w, x in enumerate(d)) == m
    return d


def nonzero_digits(cols, c):
    return sum(1 for col in cols for s in col for d in signed_digits(s, c) if d)


def edge_scalars(c):
    W, half = windows(c), 1 << (c - 1)
    out = [0, 1, R - 1, HALF_R, HALF_R + 1]                                  # the sign split
    for w in range(W):
        out += [(1 << (c * w)) - 1, 1 << (c * w), (1 << (c * w)) + 1]          # all < 2^253 < r for c = 8 .. 15
    k = max(w for w in range(W) if (1 << (c * w)) <= HALF_R)
    minus_ones = (1 << (c * k)) - sum(1 << (c * w) for w in range(k))         # every window below k is half - 1 after biasing (digit -1)
    assert signed_digits(minus_ones, c)[:k + 1] == [-1] * k + [1]
    out += [minus_ones, R - minus_ones]
    for w in range(W):                                                       # digit -half, carry into the next window
        v = 1 << (c * w + c - 1)
        if v <= HALF_R:
            assert signed_digits(v, c)[w] == -half
            out += [v, R - v]
    top = (1 << 252) - 1                                                     # every window full, the carry runs to window W - 1
    assert top < HALF_R
    out += [top, R - top, HALF_R - 1, HALF_R + 2]
    return out


def columns(c, n, n_cols, seed):
    """n_cols columns of n scalars (Python integers).  Column 0: the edge scalars, the first ones in the first and last rows of the
    chunks (P = 128 or 256), the rest from row 1 on, random full-width values between; column 1: 8-bit and 0/1 cells (wtop = 2) and
    short negatives; column 2: all zeros; further columns: the same kinds mixed row by row, and a lone non-zero scalar in the last row."""
    rng = np.random.default_rng(seed)

    def full():
        return int.from_bytes(rng.bytes(32), "little") % R

    def short():
        return [int(rng.integers(0, 2)), int(rng.integers(0, 256)), R - int(rng.integers(1, 256))][int(rng.integers(0, 3))]

    edge = edge_scalars(c)
    assert len(edge) <= n - 8
    col0 = [full() for _ in range(n)]
    first = [0, 127, 128, 255] + ([n - 1] if n - 1 != 255 else [])
    spots = first + [i for i in range(n) if i not in first]
    for pos, s in zip(spots, edge):
        col0[pos] = s
    cols = [col0, [short() for _ in range(n)], [0] * n]
    lone = [0] * n
    lone[n - 1] = edge[2 + len(cols) % 3]
    cols.append(lone)
    while len(cols) < n_cols:
        j = len(cols)
        if j % 4 == 0:
            cols.append(col0[j:] + col0[:j])                                  # the edge scalars at other rows and lanes
        elif j % 4 == 1:
            cols.append([full() if (i + j) % 5 == 0 else short() for i in range(n)])
        elif j % 4 == 2:
            cols.append([full() for _ in range(n)])
        else:
            cols.append([0] * (n - 1) + [full()])
    if n_cols == 1:
        return cols[:1]
    if n_cols == 3:
        return [cols[0], cols[1], cols[2]] if n == N_FULL else [cols[0], cols[3], cols[2]]
    return cols[:n_cols]


def _bases(n, seed):
    b = orc.g1_powers(orc.ints_to_mont([seed * 7919 + 3])[0], orc.ints_to_mont([0x1234567 + seed])[0], n)
    b[n // 5] = 0                                                             # an identity base: its table rows are identities
    return b


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


class Runs:
    """per width: the two bases with their tables, made once (4.5 GB at 15 bits and n = 256: the budget is raised for that width alone
    and the environment put back); per case: the GPU result, the additions it took, the oracle's result, the digits' count"""

    def __init__(self, ctx):
        self.ctx, self.width, self.bases, self.done = ctx, None, {}, {}

    def close(self):
        for B, _ in self.bases.values():
            B.destroy()
        self.bases = {}

    def basis(self, width, n):
        import zk_fhe_amd as zk
        if width != self.width:
            self.close()
            self.width = width
        if n not in self.bases:
            pts = _bases(n, 100 + n)
            saved = {k: os.environ.get(k) for k in ("ZKFHE_TABLE_GB", "ZKFHE_TABLE_BITS")}
            os.environ["ZKFHE_TABLE_BITS"] = str(width)
            os.environ["ZKFHE_TABLE_GB"] = "8" if width == 15 else "2"
            try:
                B = zk.Basis(self.ctx, pts)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            assert B.has_table and self.ctx.lib.zkfhe_basis_table_bits(B.h, None) == width
            self.bases[n] = (B, pts)
        return self.bases[n]

    def msm_counted(self, B, S):
        self.ctx.prof_enable(True)
        try:
            got = self.ctx.msm(B, S)
            adds = self.ctx.prof_read(0)["ops"] + self.ctx.prof_read(2)["ops"]   # slot of a wide call, slot of a call of a few columns
        finally:
            self.ctx.prof_enable(False)
        return got, int(adds)

    def case(self, width, n, n_cols):
        key = (width, n, n_cols)
        if key not in self.done:
            B, pts = self.basis(width, n)
            cols = columns(width, n, n_cols, seed=1000 * width + 10 * n_cols + n)
            S = np.stack([orc.ints_to_mont(col) for col in cols])
            got, adds = self.msm_counted(B, S)
            self.done[key] = {"got": got, "adds": adds, "want": orc.msm(S, pts), "digits": nonzero_digits(cols, width), "S": S, "cols": cols}
        return self.done[key]


@pytest.fixture(scope="module")
def runs(ctx):
    r = Runs(ctx)
    yield r
    r.close()


# width-major: one pair of tables alive at a time; 13 bits last, whose tables test C uses again
CASES = [(w, n, k) for w in (9, 11, 15, GENERIC, 13) for n in (N_FULL, N_PART) for k in N_COLS]
assert sorted(set(w for w, _, _ in CASES)) == sorted(SPECIALISED + (GENERIC,))


@pytest.mark.parametrize("width,n,n_cols", CASES)
def test_sums_equal_the_oracle(runs, width, n, n_cols):
    """A: the affine outputs, column by column; the all-zero column is the identity"""
    r = runs.case(width, n, n_cols)
    assert np.array_equal(r["got"], r["want"])
    if n_cols >= 3:
        assert not r["got"][2].any()


@pytest.mark.parametrize("width,n,n_cols", CASES)
def test_additions_equal_the_nonzero_digits(runs, width, n, n_cols):
    """B: one mixed addition per non-zero signed digit, no more and no fewer (a condition, not a tolerance)"""
    r = runs.case(width, n, n_cols)
    print("width %d, n = %d, %d column(s): %d additions, %d non-zero digits" % (width, n, n_cols, r["adds"], r["digits"]))
    assert r["adds"] == r["digits"]


def test_specialised_equals_generic(runs, monkeypatch):
    """C: the same 17 mixed columns of 300 through k_msm_table<false, 13> and, under ZKFHE_TABLE_GENERIC=1, through the run-time width
    of the same table: the same points and the same number of additions (and the oracle's, by A)."""
    r = runs.case(13, N_PART, 17)
    B, _ = runs.basis(13, N_PART)
    monkeypatch.setenv("ZKFHE_TABLE_GENERIC", "1")
    got, adds = runs.msm_counted(B, r["S"])
    monkeypatch.delenv("ZKFHE_TABLE_GENERIC")
    assert np.array_equal(got, r["got"]) and np.array_equal(got, r["want"])
    assert adds == r["adds"] == r["digits"]
