"""The MSM kernels on the lazy signed-limb point arithmetic (csrc/fq29.hip.hpp, the generated signed products of mont29_tied.inc) against
the oracle MSM, bit-exact: the table-sum path with few columns (one partial per visit) and many (256 partials per visit), at the
digit widths the table budgets produce, and the bucket pipeline one size above the table limit.  The bases are brought by the
caller, so duplicated and negated points make the doubling and the cancellation paths of the additions run on the device:

    bases = [ G0 | G0 | G2 | -G2 ]   four blocks of 256 points

A chunk of a column is at most 256 consecutive points and the entries of a chunk go to the threads in order, so thread t (or slot t of
the partial lists, if two workgroups took the chunks) meets point t of every block it has a non-zero scalar for: the same point twice
is a doubling through the addition, a point and its negative a cancellation -- by the bases or by the sign of the scalar.  In the
bucket pipeline equal scalars put such a pair into one bucket.
Run on the MI355X box:  python -m pytest tests/test_gpu_msm_lazy.py -m gpu -q
"""
import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref

pytestmark = pytest.mark.gpu
BLOCK = 256
N = 4 * BLOCK


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def _bases():
    g = orc.g1_powers(orc.ints_to_mont([7919 * 11 + 3])[0], orc.ints_to_mont([0x1234567 + 11])[0], 2 * BLOCK)
    g0, g2 = g[:BLOCK], g[BLOCK:]
    neg = orc.points_to_arr([None if p is None else (p[0], (pyref.Q - p[1]) % pyref.Q) for p in orc.arr_to_points(g2)])
    bases = np.concatenate([g0, g0, g2, neg])
    bases[BLOCK + 17] = 0   # an identity base (its twin in block 0 then stands alone)
    return bases


def _columns(rng):
    R = pyref.R
    z = [0] * BLOCK
    s = [int(rng.integers(1, 1 << 8)) for _ in range(BLOCK)]              # one digit each
    w = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(BLOCK)]   # full width: every window
    cols = [
        [int.from_bytes(rng.bytes(32), "little") % R for _ in range(N)],  # full-width values
        [0] * N,                                                          # zeros: the identity
        [1] * N,                                                          # ones
        [int(rng.integers(0, 256)) for _ in range(N)],                    # 8-bit cells
        [R - 1] * N,                                                      # r - 1: every entry negated
        s + s + z + z,                                                    # the same point twice: doubling
        z + z + s + s,                                                    # a point and its negative: cancellation, the sum is the identity
        s + [R - v for v in s] + z + z,                                   # cancellation by the sign of the scalar
        z + z + s + [R - v for v in s],                                   # doubling by the sign of the scalar
        w + w + z + z,                                                    # doubling in every window
        z + z + w + w,                                                    # cancellation in every window
    ]
    return np.stack([orc.ints_to_mont(c) for c in cols])


def _wide(S, n_cols):
    """n_cols columns: the given ones, then copies rotated by two blocks (the pairs stay pairs: a doubling becomes a cancellation)"""
    k = len(S)
    return np.stack([np.roll(S[j % k], 2 * BLOCK * (j // k), axis=0) for j in range(n_cols)])


@pytest.mark.parametrize("bits", [0, 13, 15])
def test_table_sum_with_doublings_and_cancellations(ctx, monkeypatch, bits):
    """k_msm_table<true> (11 columns, a butterfly and one partial per visit) and k_msm_table<false> (33 columns, 256 partials per visit)
    and their folds: 13- and 15-bit digits (what the default and the service budget give a 2^13 basis) and the width a 2 GB budget
    gives this basis; twice, since the ticket counters reset themselves."""
    import zk_fhe_amd as zk
    if bits:
        monkeypatch.setenv("ZKFHE_TABLE_BITS", str(bits))
        monkeypatch.setenv("ZKFHE_TABLE_GB", "48")
    else:
        monkeypatch.delenv("ZKFHE_TABLE_BITS", raising=False)
        monkeypatch.setenv("ZKFHE_TABLE_GB", "2")
    rng = np.random.default_rng(1300 + bits)
    bases = _bases()
    S = _columns(rng)
    B = zk.Basis(ctx, bases)
    assert B.has_table
    want = orc.msm(S, bases)
    assert not want[1].any() and not want[6].any() and not want[10].any()      # the identity columns
    assert want[5].any() and want[8].any() and want[9].any()
    for _ in range(2):
        assert np.array_equal(ctx.msm(B, S), want)
    Sw = _wide(S, 33)
    want_w = orc.msm(Sw, bases)
    assert np.array_equal(want_w[:len(S)], want)
    for _ in range(2):
        assert np.array_equal(ctx.msm(B, Sw), want_w)
    aff, raw = ctx.msm_xyzz(B, S)
    assert np.array_equal(aff, want)
    assert not raw[6, 8:].any()                                                # a cancelled column is the identity: ZZ = ZZZ = 0
    B.destroy()


@pytest.mark.parametrize("n_cols", [11, 33])
def test_bucket_path_above_the_table_limit(ctx, monkeypatch, n_cols):
    """A budget of 1/8 GB holds an 8-bit table for 512 points and none for these 1024: the basis takes the bucket pipeline
    (k_msm_accumulate, the bucket tails), where equal scalars put a point and its twin, or its negative, into one bucket."""
    import zk_fhe_amd as zk
    monkeypatch.delenv("ZKFHE_TABLE_BITS", raising=False)
    monkeypatch.setenv("ZKFHE_TABLE_GB", "0.125")
    rng = np.random.default_rng(77 + n_cols)
    bases = _bases()
    S = _wide(_columns(rng), n_cols)
    B = zk.Basis(ctx, bases)
    assert not B.has_table
    want = orc.msm(S, bases)
    assert not want[6].any() and want[5].any()
    assert np.array_equal(ctx.msm(B, S), want)
    B.destroy()
