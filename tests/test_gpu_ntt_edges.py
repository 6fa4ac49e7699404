"""Structured columns through every NTT kernel, bit for bit against the CPU oracle: constant columns, alternating columns, single
entries, geometric columns whose transform is ONE spike and exact zeros, and the images of "every output r - 1".  Random columns
never produce an output, or a value between two passes, that is = 0 or = -1 mod r: these do, so lz_store_weak / fr29_canonical
turning the representative r into 0, lz_weak on a negative value and butterflies whose inputs are all r - 1 are on the path.
The patterns and the proof of what they promise live in tests/test_product_bounds_host.py (no GPU); where the transform of a column
is known in closed form it is asserted next to the oracle's, so a wrong oracle cannot agree with a wrong kernel.
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import numpy as np
import pytest

from oracle import binding as orc
from oracle import pyref
from tests.test_product_bounds_host import LARGE_SIZE_PATTERNS, R, W_ALT, ntt_patterns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def words(col):
    """a column of words (python integers) as the (n, 4) array in memory: the words ARE the standard form, nothing is converted"""
    n = len(col)
    if col.count(col[0]) == n:
        return np.tile(orc.ints_to_arr(col[:1]), (n, 1))
    if col[:2] * (n // 2) == col:
        return np.tile(orc.ints_to_arr(col[:2]), (n // 2, 1))
    if col.count(0) >= n // 2:
        a = np.zeros((n, 4), dtype=np.uint64)
        idx = [i for i, w in enumerate(col) if w]
        a[idx] = orc.ints_to_arr([col[i] for i in idx])
        return a
    return orc.ints_to_arr(col)


def batch(log_n, only=None):
    pats = list(ntt_patterns(log_n, only=only))
    return pats, np.stack([words(col) for _, col, _, _ in pats])


def run_to(ctx, a, log_n, inverse):
    """out of place: the source must come back untouched"""
    n_cols, n = a.shape[0], a.shape[1]
    src, dst = ctx.to_device(a), ctx.alloc(n_cols * n * 32)
    ctx.ntt_to_dev(src, dst, n_cols, log_n, inverse=inverse)
    got = dst.download(shape=(n_cols, n, 4))
    assert np.array_equal(src.download(shape=(n_cols, n, 4)), a), "ntt_to_dev wrote to its source"
    src.free(), dst.free()
    return got


def check_closed_forms(pats, got, which, log_n):
    """zero count, spike position and spike value from the closed form -- not from the oracle"""
    n = 1 << log_n
    for c, pat in enumerate(pats):
        closed = pat[which]
        if closed is None:
            continue
        nonzero = np.flatnonzero(got[c].any(axis=1))
        if isinstance(closed, tuple):
            assert len(nonzero) == n and np.array_equal(got[c], np.tile(orc.ints_to_arr([closed[1]]), (n, 1))), (pat[0], which)
        else:
            assert list(nonzero) == sorted(closed), "%s: %d zeros, expected %d" % (pat[0], n - len(nonzero), n - len(closed))
            assert np.array_equal(got[c][nonzero], orc.ints_to_arr([closed[k] for k in sorted(closed)])), (pat[0], which)


# 1..13: the tiles 2^3..2^12 (below: the small kernels) and k_ntt13; 14, 15: k_dif_stage / k_dif_fused above the tile; 16: k_dif8_one;
# 17: the LDS pass (k_dif_lds); 19: k_dif8_two.  From 2^16 on six columns: LARGE_SIZE_PATTERNS (the constant r - 1, the alternating
# (w, r - w), the single r - 1 at 0, the spike-producing c omega^(-(n/2+1) j), the inverse image of "all r - 1", the random control).
@pytest.mark.parametrize("log_n", list(range(1, 18)) + [19])
def test_structured_columns(ctx, log_n):
    pats, a = batch(log_n, only=LARGE_SIZE_PATTERNS if log_n >= 16 else None)
    assert len(pats) == (6 if log_n >= 16 else 18)
    for inverse in (False, True):
        want = orc.ntt(a, log_n, inverse)
        check_closed_forms(pats, want, 3 if inverse else 2, log_n)   # the oracle itself against the closed forms
        got = ctx.ntt(a, log_n, inverse)
        bad = [pats[c][0] for c in range(len(pats)) if not np.array_equal(got[c], want[c])]
        assert not bad, "in place, inverse=%s: %s" % (inverse, bad)
        check_closed_forms(pats, got, 3 if inverse else 2, log_n)
        got = run_to(ctx, a, log_n, inverse)
        bad = [pats[c][0] for c in range(len(pats)) if not np.array_equal(got[c], want[c])]
        assert not bad, "out of place, inverse=%s: %s" % (inverse, bad)


@pytest.mark.parametrize("n_cols", [9, 37])
def test_structured_columns_in_ragged_groups_of_the_2_13_tile(ctx, n_cols):
    """k_ntt13 places columns in groups of eight: 9 and 37 leave the last group ragged, with structured columns in it"""
    log_n = 13
    pats, a18 = batch(log_n)
    idx = [(5 * i + 2) % 18 for i in range(n_cols)]   # the last, ragged group gets other patterns than the first
    a = a18[idx]
    p = [pats[i] for i in idx]
    for inverse in (False, True):
        want = orc.ntt(a18, log_n, inverse)[idx]
        for got in (ctx.ntt(a, log_n, inverse), run_to(ctx, a, log_n, inverse)):
            bad = [(c, p[c][0]) for c in range(n_cols) if not np.array_equal(got[c], want[c])]
            assert not bad, "inverse=%s: %s" % (inverse, bad)
            check_closed_forms(p, got, 3 if inverse else 2, log_n)


COSET_PATTERNS = ("const r-1", "c omega^(-1 j)", "alternating (w, r-w)")
# the same three as s rho^j: (s, rho)
COSET_GEOMETRIC = {
    "const r-1": lambda log_n: (R - 1, 1),
    "c omega^(-1 j)": lambda log_n: (R - 1, pow(pyref.root_of_unity(log_n), -1, R)),
    "alternating (w, r-w)": lambda log_n: (W_ALT, R - 1),
}


def COSET_SAMPLES(m):
    """both ends, the middle, and 24 seeded indices of the m extended values"""
    rng = np.random.default_rng(m)
    return sorted({0, 1, m // 2 - 1, m // 2, m - 2, m - 1, *(int(k) for k in rng.integers(0, m, 24))})


@pytest.mark.parametrize("log_n,lef", [(8, 2), (13, 1), (13, 2), (14, 2), (16, 1)])
def test_coset_ntt_structured_columns(ctx, log_n, lef):
    """k_ext_combine and the coset pre-multiplication: the constant r - 1, the spike-producing column and the alternating column, forward
    (2^log_n coefficients in) and inverse (2^(log_n + lef) extended values in, in the library's [k1][k2] order)"""
    n, E = 1 << log_n, 1 << lef
    g = orc.ints_to_mont([pyref.FR_GEN])[0]
    pats, a = batch(log_n, only=COSET_PATTERNS)
    assert len(pats) == 3
    assert orc.arr_to_ints(a[0][:1]) == [R - 1]   # the words in memory are the pattern's own: nothing was converted on the way
    got = ctx.coset_ntt(a, log_n, lef, g)
    for c in range(3):
        nat = orc.coset_ntt(a[c], log_n + lef, g)  # nat[k] = f(g w_ext^k)
        assert np.array_equal(got[c], nat.reshape(n, E, 4).transpose(1, 0, 2).reshape(n * E, 4)), pats[c][0]
        # each of the three columns is s rho^j, so f(x) = s (x^n - 1) / (rho x - 1) in closed form (rho^n = 1; x = g w^k is outside
        # the subgroup, so rho x != 1): sampled outputs against Python integers, the oracle left out of it
        w_ext = pyref.root_of_unity(log_n + lef)
        s, rho = COSET_GEOMETRIC[pats[c][0]](log_n)
        for k in COSET_SAMPLES(n * E):
            x = pyref.FR_GEN * pow(w_ext, k, R) % R
            want = s * (pow(x, n, R) - 1) * pow(rho * x - 1, -1, R) % R
            assert orc.arr_to_ints(got[c][(k % E) * n + k // E][None])[0] == want, (pats[c][0], k)
    pats, ext = batch(log_n + lef, only=COSET_PATTERNS)
    back = ctx.coset_ntt(ext, log_n, lef, g, inverse=True)
    for c in range(3):
        nat = ext[c].reshape(E, n, 4).transpose(1, 0, 2).reshape(n * E, 4)   # nat[k1 + E k2] <- ext[k1][k2]
        assert np.array_equal(back[c], orc.coset_ntt(nat, log_n + lef, g, inverse=True)), pats[c][0]
