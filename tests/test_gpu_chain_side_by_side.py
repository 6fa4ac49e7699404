"""A proof's independent thin launches run side by side (grand products, SHPLONK rotation sets, H(X) with the barycentric
denominators): every merged launch against the sequence of launches it replaces, on the same inputs, word for word -- and a k = 13
proof against a context that keeps the old sequence (ZKFHE_CHAIN=serial), with the steady-state launch counts.
tests/native/chain_side_by_side_driver.hip runs both sequences: compiled once with the library's flags, run once as a child
process; the tests compare its files.  Run on the MI355X box: pytest -m gpu."""
import os
import random
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests import prover_kernel_cases as pc
from tests.test_gpu_chain_commands import oracle_k13_proof
from tests.test_gpu_prover import first_diff, oracle_k13

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "chain_side_by_side_driver.hip")
R, W, SENT = pc.R, pc.W, pc.SENT
GUARD = b"\xa5" * 32
PER = 48   # chain::PER

# ------------------------------------------------------------------------------------------------ the cases
# grand products: n = 512, u = 505; n_perm = n_advice + 2 is odd, so the last chunk is short.  (n_advice, chunk) -> n_chunks
GP = {   # case: (n_advice, chunk, n_chunks, n_lookup, permutation closes, lookups close)
    "gp_1_0": (1, 4, 1, 0, True, True),     # no lookups: one launch carries k_powers alone, the closing launch has one workgroup
    "gp_1_1": (1, 4, 1, 1, False, True),    # a copy constraint is violated
    "gp_3_1": (5, 3, 3, 1, True, True),     # chunks of 3, 3, 1; the chunk totals differ from one, their product is one
    "gp_2_3": (3, 3, 2, 3, True, False),    # chunks of 3, 2; the total of the last lookup column is not one
}
GP_N, GP_U = 512, 505
SEED = bytes(range(11, 43))
CTR_PZ = (1 << 32) + 12345   # the counter base lies above 2^32
SH_SIZES = {1: [97], 6: [1, 48, 49, 97, 48, 1], 8: [97, 1, 48, 49, 97, 49, 1, 48]}
SH = {"sh_%d_%d" % (n, ns): (n, ns) for n in (512, 8192) for ns in (1, 6, 8)}
SH_COLS = 24
EV = {"ev_512": 512, "ev_8192": 8192}


def rand_words(rng, count):
    """canonical words below 2^248, as bytes: no Python loop over the rows"""
    a = np.frombuffer(rng.bytes(count * 32), dtype=np.uint8).reshape(count, 32).copy()
    a[:, 31] = 0
    return a.tobytes()


def words_of(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


@pytest.fixture(scope="module")
def wpow():
    return {512: pc.wpow_words(9), 8192: pc.wpow_words(13)}


def gp_case(name, wp, files, lines):
    n_advice, chunk, nch, nl, perm_closes, lookups_close = GP[name]
    n, u, n_perm = GP_N, GP_U, n_advice + 2
    assert n_perm % 2 == 1 and (n_perm + chunk - 1) // chunk == nch and n_perm % chunk
    rnd = random.Random(name)
    rng = np.random.default_rng(len(name) + n_perm)
    beta, gamma, delta = (rnd.randrange(R) for _ in range(3))
    cols = [words_of(rand_words(rng, n)) for _ in range(n_perm)]   # advice columns, the constants, the instance
    dpow = [W(1)]
    for _ in range(n_perm - 1):
        dpow.append(pc.mulw(dpow[-1], delta))
    if perm_closes:
        # the identity permutation, and one pair of equal cells in the first and in the last column (the first and the last chunk)
        # exchanged: ratios and chunk totals differ from one, the product of everything is one
        sigma = [[pc.mulw(dpow[c], wp[i]) for i in range(n)] for c in range(n_perm)]
        cols[0][3] = cols[n_perm - 1][9]
        sigma[0][3], sigma[n_perm - 1][9] = sigma[n_perm - 1][9], sigma[0][3]
    else:
        sigma = [words_of(rand_words(rng, n)) for _ in range(n_perm)]
    a = [words_of(rand_words(rng, n)) for _ in range(nl)]
    table = words_of(rand_words(rng, n))
    # a lookup column closes when (la, ls) hold the rows [0, u) of (a, table) in another order: reversed
    la = [col[:u][::-1] + col[u:] for col in a]
    ls = [table[:u][::-1] + table[u:] for _ in range(nl)]
    if not lookups_close:
        la[nl - 1] = list(la[nl - 1])
        la[nl - 1][17] = (la[nl - 1][17] + 1) % R
    flat = lambda rows: pc.to_bytes([x for r in rows for x in r])   # noqa: E731
    for key, data in (("adv", flat(cols[:n_advice])), ("const", pc.to_bytes(cols[n_advice])), ("inst", pc.to_bytes(cols[n_advice + 1])), ("sigma", flat(sigma)),
                      ("wpow", pc.to_bytes(wp)), ("a", flat(a)), ("table", pc.to_bytes(table)), ("la", flat(la)), ("ls", flat(ls))):
        files["%s.%s" % (name, key)] = data
    seed = [int.from_bytes(SEED[8 * i:8 * i + 8], "little") for i in range(4)]
    lines.append("gp %s %d %d %d %d %d %s %s %s %d %d %d %d %d" % (name, n, u, n_advice, chunk, nl, pc.hexw(beta), pc.hexw(gamma), pc.hexw(delta), *seed, CTR_PZ))


def sh_case(name, wp, files, lines):
    n, ns = SH[name]
    sizes = SH_SIZES[ns]
    rnd = random.Random(name)
    rng = np.random.default_rng(n + ns)
    cols = bytearray(rand_words(rng, SH_COLS * n))
    cols[5 * n * 32:6 * n * 32] = pc.to_bytes([R - 1] * n)   # a column of r - 1 in every row
    s29 = [rnd.randrange(R) for _ in range(sum(sizes))]
    s29[0] = 0          # a zero scalar: in the first job, and ...
    s29[-1] = 0         # ... in the last one
    s29[len(s29) // 2] = R - 1
    sets = b""
    for j in range(ns):
        n_pts = 1 + (j + ns) % 4
        pts = [rnd.randrange(R) for _ in range(n_pts)] + [0] * (4 - n_pts)
        sets += pc.shset_bytes(dict(n_pts=n_pts, pts=pts, rc=[rnd.randrange(R) for _ in range(4)], vj=rnd.randrange(R), coef=0, r_u=0))
    files.update({name + ".cols": bytes(cols), name + ".s29": pc.to_bytes(s29), name + ".sets": sets, name + ".wpow": pc.to_bytes(wp)})
    lines.append("sh %s %d %d %d %s" % (name, n, SH_COLS, ns, " ".join(map(str, sizes))))


def ev_case(name, wp, files, lines):
    n = EV[name]
    rnd = random.Random(name)
    rng = np.random.default_rng(n)
    pts = [rnd.randrange(R) for _ in range(6)]
    pts[1], pts[4] = wp[37], wp[n - 1]   # two denominators are zero
    files.update({name + ".h": rand_words(rng, 3 * n), name + ".s29": pc.to_bytes([W(1) * 32 % R, rnd.randrange(R), 0]), name + ".pts": pc.to_bytes(pts),
                  name + ".wpow": pc.to_bytes(wp)})
    lines.append("ev %s %d" % (name, n))


def compile_driver(exe):
    from zk_fhe_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    t0 = time.time()
    subprocess.run([hipcc, *build.FLAGS, "-I", os.path.join(ROOT, "zk-fhe_amd", "host"), "-I", build.CSRC, SRC, "-o", exe], check=True)
    print("chain_side_by_side_driver: compiled in %.1f s" % (time.time() - t0))
    return exe


@pytest.fixture(scope="module")
def outputs(tmp_path_factory, wpow):
    """the driver's one run: 12 cases, some hundred launches; the limit of 60 s covers that step alone and leaves room for a slow disk"""
    exe = compile_driver(str(tmp_path_factory.mktemp("sbs_exe") / "chain_side_by_side_driver"))
    d = str(tmp_path_factory.mktemp("sbs_cases"))
    files, lines = {}, []
    for name in GP:
        gp_case(name, wpow[GP_N], files, lines)
    for name in SH:
        sh_case(name, wpow[SH[name][0]], files, lines)
    for name in EV:
        ev_case(name, wpow[EV[name]], files, lines)
    os.makedirs(os.path.join(d, "in"))
    os.makedirs(os.path.join(d, "out"))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    for name, data in files.items():
        with open(os.path.join(d, "in", name), "wb") as f:
            f.write(data)
    t0 = time.time()
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=60)
    print("chain_side_by_side_driver: ran in %.1f s: %s" % (time.time() - t0, r.stdout.strip()[-200:]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d cases run" % len(lines) in r.stdout

    def read(case, which, buf):
        with open(os.path.join(d, "out", "%s.%s.%s.bin" % (case, which, buf)), "rb") as f:
            return f.read()
    yield read
    shutil.rmtree(d, ignore_errors=True)


def same_and_guarded(read, case, buf, words, guard):
    """both sequences left the same bytes in the whole buffer, the guard behind its `words` rows included, and the guard is untouched"""
    old, new = read(case, "old", buf), read(case, "new", buf)
    assert len(old) == len(new) == (words + guard) * 32
    assert new[words * 32:] == GUARD * guard, "%s.%s: the rows behind the output were written" % (case, buf)
    if old != new:
        k = next(i for i in range(0, len(old), 32) if old[i:i + 32] != new[i:i + 32]) // 32
        raise AssertionError("%s.%s: word %d of %d differs: %s (sequence) / %s (side by side)" % (case, buf, k, words, old[k * 32:k * 32 + 32].hex(), new[k * 32:k * 32 + 32].hex()))
    return new


@pytest.mark.parametrize("case", list(GP))
def test_grand_products_side_by_side(outputs, case):
    """beta delta^c, both factors of every ratio, the ratios, the product columns with their blinding rows, the carries and totals and
    the two flags: six launches leave what ten left.  The flags say what the case was built to show."""
    n_advice, chunk, nch, nl, perm_closes, lookups_close = GP[case]
    n, u, cols = GP_N, GP_U, nch + nl
    same_and_guarded(outputs, case, "bd", n_advice + 2, 8)
    for buf in ("num", "den"):
        same_and_guarded(outputs, case, buf, cols * n, n)
    z = same_and_guarded(outputs, case, "z", cols * n, n)
    assert GUARD not in (z[i:i + 32] for i in range(0, cols * n * 32, 32)), "a row of a product column was left unwritten"
    totals = words_of(same_and_guarded(outputs, case, "totals", cols, 8)[:cols * 32])
    closes = np.frombuffer(same_and_guarded(outputs, case, "closes", 1, 0), dtype="<i4")
    assert list(closes[:2]) == [int(perm_closes), int(lookups_close)]
    assert closes[2:].tobytes() == b"\xa5" * 24
    # the blinding rows of the last column: the draws that follow the permutation columns' (ctr_lz = ctr_pz + n_chunks (n - u - 1))
    nb = n - u - 1
    want = pc.rng_row_words(SEED, CTR_PZ + (cols - 1) * nb, nb)
    assert words_of(z[((cols - 1) * n + u + 1) * 32:cols * n * 32]) == want
    assert all(t == pc.ONE for t in totals[nch:]) == lookups_close
    if nl and not lookups_close:
        assert all(t == pc.ONE for t in totals[nch:-1]) and totals[-1] != pc.ONE   # the last slot alone
    if nch > 1 and perm_closes:
        assert any(words_of(z[(j * n + u) * 32:(j * n + u + 1) * 32])[0] != pc.ONE for j in range(nch - 1))   # no chunk closes alone
        assert words_of(z[((nch - 1) * n + u) * 32:((nch - 1) * n + u + 1) * 32]) == [pc.ONE]


@pytest.mark.parametrize("case", list(SH))
def test_shplonk_sets_side_by_side(outputs, case):
    """1, 6 and 8 rotation sets of 1, 48, 49 and 97 members in one call: two launches leave in F and zs what up to 17 left; the partial
    sums lie in the slots the job list names and nowhere else"""
    n, ns = SH[case]
    F = same_and_guarded(outputs, case, "F", ns * n, n)
    assert GUARD not in (F[i:i + 32] for i in range(0, ns * n * 32, 32 * 61))
    zs = same_and_guarded(outputs, case, "zs", ns * n, n)
    assert outputs(case, "split", "F") == F and outputs(case, "split", "zs") == zs   # the jobs alone, k_sh_zs in a launch of its own
    slots = sum(c for c in ((m + PER - 1) // PER for m in SH_SIZES[ns]) if c > 1)
    partial = outputs(case, "new", "partial")
    assert len(partial) == 17 * n * 32
    assert partial[slots * n * 32:] == GUARD * ((17 - slots) * n)
    assert GUARD not in (partial[i:i + 32] for i in range(0, slots * n * 32, 32))


@pytest.mark.parametrize("case", list(EV))
def test_evaluation_round_side_by_side(outputs, case):
    """H(X) from its three pieces and the six rows of barycentric denominators, two of them with a zero: one launch leaves what two left"""
    n = EV[case]
    same_and_guarded(outputs, case, "H", n, n)
    bw = words_of(same_and_guarded(outputs, case, "bw", 6 * n, n)[:6 * n * 32])
    assert [i for i, x in enumerate(bw) if x == 0] == [n + 37, 4 * n + n - 1]


# ------------------------------------------------------------------------------------------------ whole proofs
@pytest.fixture(scope="module")
def k13_pair():
    """a context of the default path and one created under ZKFHE_CHAIN=serial, one k = 13 SRS with the library's default table budget
    (the path bench.py measures), one key per transcript"""
    import torch  # noqa: F401
    import zk_fhe_amd as zk
    saved = {k: os.environ.pop(k, None) for k in ("ZKFHE_TABLE_GB", "ZKFHE_TABLE_BITS", "ZKFHE_CHAIN")}
    try:
        ctx = zk.Context(0)
        os.environ["ZKFHE_CHAIN"] = "serial"
        ctx_serial = zk.Context(0)
        del os.environ["ZKFHE_CHAIN"]
        srs = zk.Srs(ctx, 13)
    finally:
        os.environ.pop("ZKFHE_CHAIN", None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    o = oracle_k13()
    keys = {}

    def key(transcript):
        if transcript not in keys:
            zcfg = zk.BfvConfig.from_pinning(o["cfgj"], transcript=transcript)
            keys[transcript] = zk.BfvProvingKey(ctx, srs, o["text_empty"], (1024, o["prm"].Q, o["prm"].T, o["prm"].B), zcfg)
        return keys[transcript]
    yield ctx, ctx_serial, key
    for pk in keys.values():
        pk.destroy()
    srs.destroy()
    ctx_serial.close()
    ctx.close()


@pytest.mark.parametrize("transcript", ["poseidon", "blake2b"])
def test_k13_proof_equals_the_serial_chain_and_is_shorter(k13_pair, monkeypatch, transcript):
    """One k = 13 proof per transcript: the bytes of a context that keeps the old sequence of launches (and the oracle's), and in steady
    state at most 64 kernel launches with the early phase-1 commitment and 59 without, no copy and no fill command."""
    ctx, ctx_serial, key = k13_pair
    monkeypatch.delenv("ZKFHE_WITNESS", raising=False)
    monkeypatch.delenv("ZKFHE_UPLOAD", raising=False)
    o = oracle_k13()
    pk = key(transcript)
    seed = b"seed-1"
    counts = {}
    proofs = {}
    for early in ("1", "0"):
        monkeypatch.setenv("ZKFHE_EARLY_P1", early)
        for name, c in (("side by side", ctx), ("serial", ctx_serial)):
            if early == "1":
                pk.prove(o["text"], b"warm-up", ctx=c)   # the first proof of a context also creates the auxiliary context's tables
            proofs[name, early] = pk.prove(o["text"], seed, ctx=c)[:2]
            counts[name, early] = c.last_proof_commands()
    print("transcript %s: %s" % (transcript, counts))
    proof_o, inst_o = oracle_k13_proof(transcript)
    for early in ("1", "0"):
        proof, inst = proofs["side by side", early]
        proof_s, inst_s = proofs["serial", early]
        assert inst == inst_s == inst_o
        assert first_diff(proof, proof_s) is None, "first differing 32-byte item: %s" % first_diff(proof, proof_s)
        assert first_diff(proof, proof_o) is None
        cmds = counts["side by side", early]
        assert cmds["kernel_launches"] <= (64 if early == "1" else 59), counts
        assert cmds["copy_commands"] == 0 and cmds["fill_commands"] == 0, counts
        assert counts["serial", early]["kernel_launches"] > cmds["kernel_launches"], counts
