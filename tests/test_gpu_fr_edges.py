"""The element-wise Fr kernels at their edges: k_fr_binop / k_fr_unop with more elements than one grid holds, so every thread takes its
grid stride, on the operand pairs where the 8 x 32-bit carries matter (a + b = r, a + b = r - 1, a - b = 0, 0 - 1, (r - 1)^2, ...); and
k_fr_batch_invert on both sides of the size at which it switches to at least 16 elements per inversion, with zeros planted where a
thread's chain begins, ends, and is zero throughout.  Against the CPU oracle, and against Python integers on the distinct operands.
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref

pytestmark = pytest.mark.gpu
R = pyref.R
RINV = pow(1 << 256, -1, R)   # the words in memory are x 2^256: the product of two words is a b / 2^256
WORDS = [0, 1, 2, R - 2, R - 1, (R - 1) // 2, (R + 1) // 2, (1 << 32) - 1, (1 << 64) - 1, 1 << 224, (1 << 253) - 1, 1 << 253]


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid(ctx):
    """every ordered pair of WORDS, tiled to two full grids of the element-wise kernels and 77 more: every thread strides, most twice"""
    n = 2 * (ctx.device_info()["num_cu"] * 8 * 256) + 77
    pa = orc.ints_to_arr([a for a in WORDS for _ in WORDS])
    pb = orc.ints_to_arr([b for _ in WORDS for b in WORDS])
    reps = -(-n // 144)
    return n, np.tile(pa, (reps, 1))[:n].copy(), np.tile(pb, (reps, 1))[:n].copy()


def test_the_operand_words_are_canonical():
    assert len(set(WORDS)) == 12 and all(0 <= w < R for w in WORDS)


@pytest.mark.parametrize("op", ["add", "sub", "mul"])
def test_binop_on_the_operand_grid_beyond_one_grid(ctx, grid, op):
    n, a, b = grid
    got = ctx.fr_binop(op, a, b)
    assert np.array_equal(got, orc.fe_binop(op, a, b))   # all n elements: a thread that does not stride leaves its later elements unwritten
    f = {"add": lambda x, y: (x + y) % R, "sub": lambda x, y: (x - y) % R, "mul": lambda x, y: x * y * RINV % R}[op]
    assert orc.arr_to_ints(got[:144]) == [f(x, y) for x in WORDS for y in WORDS]
    assert np.array_equal(got[n - 144:], np.roll(got[:144], -((n - 144) % 144), axis=0))   # the tail repeats the grid: python's figures hold there too


@pytest.mark.parametrize("s", WORDS)
def test_scale_on_the_operand_grid_beyond_one_grid(ctx, grid, s):
    n, a, _ = grid
    sw = orc.ints_to_arr([s])
    got = ctx.fr_unop("scale", a, sw)
    assert np.array_equal(got, orc.fe_binop("mul", a, np.repeat(sw, n, axis=0)))
    assert orc.arr_to_ints(got[:144:12]) == [x * s * RINV % R for x in WORDS]
    assert orc.arr_to_ints(got[n - 1:]) == [WORDS[((n - 1) % 144) // 12] * s * RINV % R]


def test_to_mont_and_from_mont_on_the_operand_grid_beyond_one_grid(ctx, grid):
    n, a, _ = grid
    m = ctx.fr_unop("to_mont", a)
    assert np.array_equal(m, orc.to_mont(a))
    assert orc.arr_to_ints(m[:144:12]) == [(x << 256) % R for x in WORDS]
    assert np.array_equal(ctx.fr_unop("from_mont", m), a)
    f = ctx.fr_unop("from_mont", a)
    assert np.array_equal(f, orc.from_mont(a))
    assert orc.arr_to_ints(f[:144:12]) == [x * RINV % R for x in WORDS]


def test_sqr_chain_on_the_operand_words(ctx):
    x = orc.ints_to_arr(WORDS * 50)   # three blocks, the last one partly filled
    want = list(WORDS)
    for _ in range(3):
        want = [w * w * RINV % R for w in want]
    assert orc.arr_to_ints(ctx.fr_unop("sqr_chain", x, 3)) == want * 50


@pytest.fixture(scope="module")
def random_words():
    """2^20 + 5 canonical words below 2^252, and as many numerators"""
    rng = np.random.default_rng(2020)
    w = rng.integers(0, 1 << 63, size=(2, (1 << 20) + 5, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(2, (1 << 20) + 5, 4), dtype=np.uint64)
    w[:, :, 3] &= np.uint64((1 << 60) - 1)
    w[0, :, 0] |= np.uint64(1)   # no accidental zero among the denominators
    return w[0], w[1]


def plant_zeros(den):
    """index 0, n - 1, a run of 40, and every index = 3 modulo ceil(n / c) for c = 8, 16, 32: whatever chunk the library picks, the thread
    that owns index 3 (elements 3, 3 + T, 3 + 2 T, ... with T = ceil(n / chunk)) has a chain of zeros only"""
    n = den.shape[0]
    zero = np.zeros(n, dtype=bool)
    zero[[0, n - 1]] = True
    zero[1000:1040] = True
    for c in (8, 16, 32):
        zero[3::-(-n // c)] = True
    den = den.copy()
    den[zero] = 0
    return den, zero


@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20, (1 << 20) + 5])
def test_batch_invert_around_the_long_array_threshold(ctx, random_words, n):
    """below 2^20 eight elements per inversion, from 2^20 on at least sixteen"""
    den, zero = plant_zeros(random_words[0][:n])
    num = random_words[1][:n]
    one = orc.ints_to_arr([(1 << 256) % R])[0]
    inv = ctx.fr_unop("batch_invert", den)
    assert np.array_equal(inv, orc.fr_batch_inv(den))
    assert not inv[zero].any() and inv[~zero].any(axis=1).all()
    prod = ctx.fr_binop("mul", den, inv)   # a a^-1 = 1 on the device itself
    assert not prod[zero].any() and (prod[~zero] == one).all()
    quot = ctx.fr_batch_invert_mul(num, den)
    assert np.array_equal(quot, orc.fe_binop("mul", num, orc.fr_batch_inv(den)))
    assert not quot[zero].any()


def test_batch_invert_of_nothing_but_zeros(ctx, random_words):
    n = 300
    den = np.zeros((n, 4), dtype=np.uint64)
    assert not ctx.fr_unop("batch_invert", den).any()
    assert not ctx.fr_batch_invert_mul(random_words[1][:n], den).any()   # the numerators come back zero
