"""What the GPU tests of the long-row NTT schedules run, in one place, and the reference they share for rows too long for the oracle.

The shape tables: tests/test_gpu_ntt_schedules.py and tests/test_gpu_ntt_rows.py take their sizes from here, and
tests/test_ntt_schedules_host.py (no GPU) holds the same tables against the plans that csrc/ntt_plan.hpp makes: every kind of pass
planned for rows of up to 2^24 points must be reached by a shape listed here, and every shape must plan what is written next to it.
A plan is spelled as in tests/native/ntt_plan_check.cpp, stages per pass: "1" k_dif_stage, "2" / "3" k_dif_fused<2> / <3>, "4L" / "5L" /
"6L" k_dif_lds<1> / <2> / <3>, "3F" / "6F" the four-step pass.

The reference: one identity in a random point that holds for a whole transform, where the oracle's own transform would take too long.
"""
import collections
import concurrent.futures

import numpy as np

from oracle import binding as orc
from oracle import pyref

R = pyref.R

# ---- the shapes --------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_ntt_schedules.py, every one in place and out of place (log_n: plan)
LARGE_SIZES = {21: "6L 2", 22: "6L 3", 23: "6L 4L", 24: "6L 5L"}   # an LDS pass with another pass behind it
STRUCTURED_SIZES = {18: "5L"}                                      # the six structured columns
# enough columns for a second trip of the first pass's grid loop: num_cu // 2 + 3 of 2^17, 2^14 and 2^15, num_cu // 4 + 3 of 2^18,
# num_cu // 32 + 3 of 2^21
LOOP_SIZES = {17: "4L", 14: "1", 15: "2", 18: "5L", 21: "6L 2"}
# zkfhe_coset_ntt_batch, (log_n, lef): the plan of the forward call, whose first pass reads the table of coset powers (2^lef rows; at
# 2^19 eight rows are more than the four-step pass takes), and the plan of the inverse call's plain row transforms, out of place
COSET_CALLS = {(17, 2): ("4L", "4L"), (18, 1): ("5L", "5L"), (19, 3): ("6L", "6F"), (20, 1): ("4L 3", "4L 3")}

# tests/test_gpu_ntt_rows.py, (log_n, lef, rows) of zk_coset_ntt_rows / zk_extend_lagrange: what the shape reaches.  Above 2^13 the
# rows are one forward out-of-place call with the table, or at 2^16 / 2^19 with at most four rows the shifts; zk_extend_lagrange runs
# a plain inverse out of place before it.
ROW_SHAPES = [
    (8, 2, 3),    # a small tile, fewer rows than cosets
    (13, 2, 3),   # zk_pre13
    (13, 1, 1),   # zk_pre13, one row
    (14, 2, 3),   # a single radix-2 stage with the table of coset powers
    (15, 2, 3),   # k_dif_fused<2> with the table
    (16, 2, 3),   # the four-step pass with shifts
    (16, 3, 5),   # a four-step size forced onto the table: more than four rows
    (17, 2, 3),   # the LDS pass with the table
    (18, 2, 3),   # k_dif_lds<2> with the table
    (19, 1, 2),   # the four-step pass of six stages with shifts
    (19, 3, 5),   # k_dif_lds<3> with the table
    (20, 2, 3),   # an LDS pass with the table and a register pass behind it
]
ROW_PLANS = {14: "1", 15: "2", (16, 3): "3F", (16, 5): "3", 17: "4L", 18: "5L", (19, 2): "6F", (19, 5): "6L", 20: "4L 3"}   # by log_n, or (log_n, rows)
PLAIN_PLANS = {14: "1", 15: "2", 16: "3F", 17: "4L", 18: "5L", 19: "6F", 20: "4L 3"}   # the inverse before them
TWO_COLUMN_ROWS = 18    # from this log_n on a row shape gets two columns, not four
# plain zkfhe_ntt_batch / zkfhe_ntt_batch_to through the same driver: the four-step sizes, which nothing above runs alone
PLAIN_CASES = {16: "3F", 19: "6F"}
# the driver's second run, with ZKFHE_NTT_LDS_PASS=0 in the child's environment: register passes of three where the LDS passes were
FALLBACK_PLAIN = {17: "3 1", 18: "3 2", 20: "3 3 1"}
FALLBACK_ROWS = {(17, 2, 3): ("3 1", "3 1"), (19, 3, 5): ("3 3", "6F")}   # with the table, and the plain inverse before it
FALLBACK_LOOP = (17, "3 1")   # num_cu // 4 + 3 columns: a second trip of k_dif_fused<3>'s grid loop


def row_plan(shape):
    log_n, _, rows = shape
    return ROW_PLANS[log_n] if log_n in ROW_PLANS else ROW_PLANS[(log_n, rows)]


Listed = collections.namedtuple("Listed", "where log_n coset lds in_place passes")


def listed_shapes():
    """every long-row call that the GPU tests make: which test, and the arguments of ntt_plan() with the plan claimed above"""
    out = []

    def plain(where, log_n, passes, lds=1, routes=(0, 1)):
        out.extend(Listed(where, log_n, "none", lds, r, passes) for r in routes)

    for log_n, passes in LARGE_SIZES.items():
        plain("test_gpu_ntt_schedules::test_large_rows", log_n, passes)
    for log_n, passes in STRUCTURED_SIZES.items():
        plain("test_gpu_ntt_schedules::test_structured_columns", log_n, passes)
    for log_n, passes in LOOP_SIZES.items():
        plain("test_gpu_ntt_schedules::test_second_trip_of_the_grid_loop", log_n, passes)
    for (log_n, lef), (fwd, inv) in COSET_CALLS.items():
        out.append(Listed("test_gpu_ntt_schedules::test_coset_call", log_n, "table", 1, 0, fwd))
        plain("test_gpu_ntt_schedules::test_coset_call", log_n, inv, routes=(0,))
    for s in ROW_SHAPES:
        if s[0] > 13:
            shifts = s[0] in (16, 19) and s[2] <= 4
            out.append(Listed("test_gpu_ntt_rows::test_coset_rows_and_extend_lagrange", s[0], "shifts" if shifts else "table", 1, 0, row_plan(s)))
            plain("test_gpu_ntt_rows::test_coset_rows_and_extend_lagrange", s[0], PLAIN_PLANS[s[0]], routes=(0,))
    for log_n, passes in PLAIN_CASES.items():
        plain("test_gpu_ntt_rows::test_plain_transforms", log_n, passes)
    for log_n, passes in list(FALLBACK_PLAIN.items()) + [FALLBACK_LOOP]:
        plain("test_gpu_ntt_rows::test_fallback_plain_transforms", log_n, passes, lds=0)
    for s, (passes, inv) in FALLBACK_ROWS.items():
        out.append(Listed("test_gpu_ntt_rows::test_fallback_coset_rows_and_extend_lagrange", s[0], "table", 0, 0, passes))
        plain("test_gpu_ntt_rows::test_fallback_coset_rows_and_extend_lagrange", s[0], inv, lds=0, routes=(0,))
    return out


# ---- columns -----------------------------------------------------------------------------------------------------------------------
def random_words(seed, n):
    """(n, 4) canonical words, uniform below 2^252 < r: a random column of a length at which a Python integer per word costs too much"""
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) << np.uint64(1)
    a[:, 3] >>= np.uint64(4)
    return a


def const_words(w, n):
    return np.tile(orc.ints_to_arr([w]), (n, 1))


# ---- the reference for rows beyond the oracle's reach -----------------------------------------------------------------------------
_pool = concurrent.futures.ThreadPoolExecutor(8)   # the oracle's calls release the interpreter lock
CHUNK = 1 << 18


def _m(v):
    return orc.ints_to_mont([v % R])[0]


def _horner_sum(a, x):
    """sum_k a[k] x^k (a Python integer), the chunks side by side"""
    n = len(a)
    parts = list(_pool.map(lambda s: orc.mont_to_ints(orc.fr_horner(a[s:s + CHUNK], _m(x))[None])[0], range(0, n, CHUNK)))
    return sum(p * pow(x, s, R) for p, s in zip(parts, range(0, n, CHUNK))) % R


def transform_identity_holds(x, X, omega, c, rho, g=1):
    """Whether X[k] = c sum_i x[i] (g omega^k)^i for all k < N = len(X) at once (x has n <= N entries, omega^N = 1), tested at the
    point rho:   sum_k rho^k X[k] = c sum_i x[i] g^i (rho^N - 1) / (rho omega^i - 1),   since sum_k (rho omega^i)^k is that quotient.
    Both sides are linear in the words, so x and X are the arrays as they lie in memory.  omega, c, rho, g: Python integers.
      forward NTT: omega = omega_N, c = 1;   inverse: omega = omega_N^-1, c = N^-1;   coset extension: omega = omega_N, g the shift,
      X in natural order (X[k] = f(g omega^k)).
    For X wrong in any word the two sides are different polynomials of degree < N in rho: a random rho hides that with probability
    at most N / r.  Uses the oracle's field arithmetic only (fr_horner, fr_powers, fr_add_scalar, fr_batch_inv, fr_mul, fr_scale)."""
    x, X = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(X, dtype=np.uint64).reshape(-1, 4)
    n, N = len(x), len(X)
    assert n <= N and pow(omega, N, R) == 1 and pow(rho, N, R) != 1
    lhs = _horner_sum(X, rho)

    def part(s):
        m = min(CHUNK, n - s)
        den = orc.fr_add_scalar(orc.fr_powers(_m(rho * pow(omega, s, R)), _m(omega), m), _m(R - 1))   # rho omega^i - 1, never 0
        t = orc.fr_mul(x[s:s + m], orc.fr_batch_inv(den))
        if g != 1:
            t = orc.fr_mul(t, orc.fr_powers(_m(pow(g, s, R)), _m(g), m))
        return orc.mont_to_ints(orc.fr_horner(t, _m(1))[None])[0]

    total = sum(_pool.map(part, range(0, n, CHUNK))) % R
    rhs = orc.mont_to_ints(orc.fr_scale(_m(total)[None], _m(c * (pow(rho, N, R) - 1))))[0]
    return lhs == rhs


def ntt_identity_holds(x, X, log_n, inverse, rho):
    w = pyref.root_of_unity(log_n)
    return transform_identity_holds(x, X, pow(w, -1, R) if inverse else w, pow(1 << log_n, -1, R) if inverse else 1, rho)


def point(seed):
    """a point for the identity, from a seed: the test's outcome does not change from run to run"""
    return int.from_bytes(np.random.default_rng(seed).bytes(40), "little") % R
