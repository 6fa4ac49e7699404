"""What the throughput profile changes below a proof, called directly on a context created under ZKFHE_PROFILE=throughput: the batch
inversion with its longer groups from 2^17 elements on (zkfhe_fr_batch_invert, zkfhe_fr_batch_invert_mul) against pow(x, r - 2, r),
and the table sums of a few columns with chunks of 256 points (k_msm_table<true>) against the bucket pipeline on the same points.
Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref
from tests.test_gpu_parity import _bases

pytestmark = pytest.mark.gpu
R = pyref.R
WIDE = 1 << 17            # csrc/core.hip BI_WIDE: from here on a thread takes the profile's group, below it 8
GROUPS = (8, 16, 32, 64)  # group sizes the kernel may be run at: the zeros below are placed for each of them


@pytest.fixture(scope="module")
def ctx():
    """a context of the throughput profile: the variable is read when the context is created (and again by every proof)"""
    import os
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    saved = {k: os.environ.pop(k, None) for k in ("ZKFHE_PROFILE", "ZKFHE_BI_CHUNK")}
    os.environ["ZKFHE_PROFILE"] = "throughput"
    try:
        c = zk.Context(0)
    finally:
        del os.environ["ZKFHE_PROFILE"]
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    yield c
    c.close()


@pytest.fixture(scope="module")
def field():
    """WIDE + 37 non-zero values and their inverses by pow(x, r - 2, r), made once: every case below reads a prefix of them.  4099
    distinct values, repeated: the period is prime to every stride a thread's group can have, so no group sees a value twice"""
    rng = np.random.default_rng(1717)
    base = [int.from_bytes(rng.bytes(32), "little") % R or 1 for _ in range(4099)]
    base_inv = [pow(v, R - 2, R) for v in base]
    return [base[i % 4099] for i in range(WIDE + 37)], [base_inv[i % 4099] for i in range(WIDE + 37)]


def zero_places(n):
    """indices that are the first and the last element of a thread's strided group, and one whole group, for every group size:
    thread t of T = ceil(n / g) owns t, t + T, t + 2 T, ... below n"""
    z = set()
    for g in GROUPS:
        T = (n + g - 1) // g
        t = min(5, T - 1)
        own = list(range(t, n, T))
        z.update((own[0], own[-1]))          # first and last of thread t's group
        z.update(range(T - 1, n, T))         # thread T - 1: every element of its group, the only one where the group has one
    return sorted(z)


@pytest.mark.parametrize("n", [1, 5, WIDE - 1, WIDE, WIDE + 1, WIDE + 37])
def test_batch_invert_both_group_sizes(ctx, field, n):
    """Lengths of a few elements, just below 2^17 (groups of 8) and from 2^17 on (the profile's group; 2^17 + 1 and 2^17 + 37 are no
    multiple of any group size, so the last threads own one element fewer).  Zeros stay zero and take nothing from their group."""
    x, inv = field
    den, want = list(x[:n]), list(inv[:n])
    for i in ([0] if n == 1 else zero_places(n) if n > 8 else [0, n - 1]):
        den[i] = want[i] = 0
    got = ctx.fr_unop("batch_invert", orc.ints_to_mont(den))
    assert np.array_equal(got, np.asarray(orc.ints_to_mont(want)).reshape(got.shape))


@pytest.mark.parametrize("n", [5, WIDE - 1, WIDE + 37])
@pytest.mark.parametrize("num_kind", ["random", "zeros", "r-1"])
def test_batch_invert_mul_both_group_sizes(ctx, field, n, num_kind):
    """num[i] * den[i]^-1 in the same pass, zero where den[i] = 0: a random numerator, one of zeros and one of r - 1 (= -1: the
    quotient is the negated inverse)"""
    x, inv = field
    den, dinv = list(x[:n]), list(inv[:n])
    for i in (zero_places(n) if n > 8 else [0, n - 1]):
        den[i] = dinv[i] = 0
    if num_kind == "random":
        num = x[37:37 + n] if n + 37 <= len(x) else x[-n:][::-1]
    else:
        num = [0 if num_kind == "zeros" else R - 1] * n
    want = [a * b % R for a, b in zip(num, dinv)]
    got = ctx.fr_batch_invert_mul(orc.ints_to_mont(num), orc.ints_to_mont(den))
    assert np.array_equal(got, np.asarray(orc.ints_to_mont(want)).reshape(got.shape))


@pytest.mark.parametrize("n,n_cols,bits", [(256, 1, 8), (1000, 3, 8), (1000, 3, 9), (8192, 1, 8), (8192, 3, 9)])
def test_few_column_table_sums_at_chunks_of_256(ctx, monkeypatch, n, n_cols, bits):
    """The 1- and 3-column cases of test_msm_table_path at n = 8192, 1000 and 256 with 8- and 9-bit tables, on the throughput
    context: such calls keep chunks of 256 points (32 visits per column at n = 8192 instead of 64, four at n = 1000 with a ragged
    last one, one at n = 256).  Called twice -- the ticket counters must reset themselves -- and against the bucket pipeline."""
    import zk_fhe_amd as zk
    monkeypatch.setenv("ZKFHE_TABLE_BITS", str(bits))
    monkeypatch.setenv("ZKFHE_TABLE_GB", "48")
    rng = np.random.default_rng(31 * n + n_cols)
    bases = _bases(n, seed=n + n_cols)
    bases[n // 5] = 0
    sc = [[int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)] for _ in range(n_cols)]
    sc[0][:8] = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, 2, 8, R - 8]
    if n_cols > 1:
        sc[1] = [int(rng.integers(0, 1 << 29)) if i % 3 else (R - int(rng.integers(1, 1000))) for i in range(n)]
    if n_cols > 2:
        sc[2] = [[0, 1, 536870908][int(rng.integers(0, 3))] for _ in range(n)]
    S = np.stack([orc.ints_to_mont(col) for col in sc])
    B = zk.Basis(ctx, bases)
    assert B.has_table
    Bb = zk.Basis(ctx, bases, 11)
    assert not Bb.has_table
    want = ctx.msm(Bb, S)
    assert np.array_equal(want, orc.msm(S, bases))
    for _ in range(2):
        assert np.array_equal(ctx.msm(B, S), want)
    B.destroy()
    Bb.destroy()
