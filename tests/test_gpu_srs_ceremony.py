"""An SRS from a ceremony's monomial powers (zkfhe_srs_from_monomial, zkfhe_srs_load_downsized) and the structure check
(zkfhe_srs_check), on the GPU.  Everything is compared as bytes: params files, key digests, proofs."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import circuit_ref as C
from oracle import halo2_ref as H
from tests.test_proof_oracle import synth_input

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    c = zk.Context(0)
    yield c
    c.close()


def read_params(path):
    """(k, g, g_lagrange, tail) of a RawBytes params file"""
    blob = open(path, "rb").read()
    k = int.from_bytes(blob[:4], "little")
    n = 1 << k
    assert len(blob) == 4 + 128 * n + 256
    g = np.frombuffer(blob, dtype=np.uint64, count=8 * n, offset=4).reshape(n, 8).copy()
    gl = np.frombuffer(blob, dtype=np.uint64, count=8 * n, offset=4 + 64 * n).reshape(n, 8).copy()
    return k, g, gl, blob[-256:]


@pytest.fixture(scope="module")
def files(ctx, tmp_path_factory):
    """the seeded setup at k = 10 and k = 9, saved once: {"a": k = 10 file, "b": k = 9 file, "g2": (G2, s G2) of both}"""
    import zk_fhe_amd as zk
    d = tmp_path_factory.mktemp("srs")
    a, b = str(d / "k10.srs"), str(d / "k9.srs")
    s10, s9 = zk.Srs(ctx, 10), zk.Srs(ctx, 9)
    s10.save(a), s9.save(b)
    g2 = s9.g2()
    assert g2 == s10.g2()
    s10.destroy(), s9.destroy()
    return {"a": a, "b": b, "g2": g2, "dir": d}


def same_file(p, q):
    return open(p, "rb").read() == open(q, "rb").read()


def test_load_downsized_equals_the_seeded_setup(ctx, files):
    import zk_fhe_amd as zk
    c = str(files["dir"] / "c.srs")
    srs = zk.Srs.load_downsized(ctx, files["a"], 9)
    srs.save(c)
    assert srs.check(SEED) == 0 and srs.g2() == files["g2"]
    srs.destroy()
    assert same_file(files["b"], c)
    # the file's own k: nothing is cut, g_lagrange is still recomputed
    srs = zk.Srs.load_downsized(ctx, files["a"], 10)
    srs.save(c)
    srs.destroy()
    assert same_file(files["a"], c)


def test_from_monomial_equals_the_seeded_setup(ctx, files):
    import zk_fhe_amd as zk
    _, g10, _, _ = read_params(files["a"])
    c = str(files["dir"] / "m.srs")
    srs = zk.Srs.from_monomial(ctx, 9, g10, *files["g2"])
    srs.save(c)
    srs.destroy()
    assert same_file(files["b"], c)
    # without the G2 half: an SRS to prove with, nothing to save or check
    srs = zk.Srs.from_monomial(ctx, 9, g10[:512])
    with pytest.raises(zk.ZkfheError, match="no G2 half"):
        srs.save(c)
    with pytest.raises(zk.ZkfheError, match="srs_check: the SRS has no G2 half"):
        srs.check(SEED)
    srs.destroy()


def test_key_and_proof_under_the_downsized_srs(ctx, files):
    """the toy circuit of test_external_srs_points (N = 8, k = 9): same key digest, same proof bytes as under zk.Srs(ctx, 9)"""
    import zk_fhe_amd as zk
    prm = C.BfvParams(N=8)
    inp = synth_input(8, prm.Q, prm.T, prm.B, 1)
    hcfg = H.auto_config(9, 9, H.BfvCircuit(inp, prm))
    zcfg = zk.BfvConfig(9, hcfg.n_gate0, hcfg.n_gate1, hcfg.n_lookup, hcfg.n_rlc, 9)
    out = []
    for srs in (zk.Srs(ctx, 9), zk.Srs.load_downsized(ctx, files["a"], 9)):
        pk = zk.BfvProvingKey(ctx, srs, json.dumps(inp), (8, prm.Q, prm.T, prm.B), zcfg)
        out.append((pk.info(), pk.prove(json.dumps(inp), b"ext")[0]))
        pk.destroy()
        srs.destroy()
    assert out[0] == out[1]


@pytest.mark.parametrize("k", [9, 13])
def test_check_passes_a_seeded_srs(ctx, k):
    import zk_fhe_amd as zk
    srs = zk.Srs(ctx, k)
    assert srs.check(SEED) == 0
    if k == 9:
        assert srs.check() == 0          # the OS's entropy
        srs.drop_host_copy()             # g[0] then comes from the device tables
        assert srs.check(SEED) == 0
    srs.destroy()


def tampered(ctx, files, g=None, gl=None, g2=None):
    """the k = 9 setup with one half replaced, through from_points + set_g2"""
    import zk_fhe_amd as zk
    _, g0, gl0, _ = read_params(files["b"])
    srs = zk.Srs.from_points(ctx, 9, g0 if g is None else g, gl0 if gl is None else gl)
    srs.set_g2(*(files["g2"] if g2 is None else g2))
    try:
        return srs.check(SEED)
    finally:
        srs.destroy()


def test_check_finds_a_wrong_power(ctx, files):
    """g[5] := g[6], with g_lagrange the Lagrange form of that g: the powers check alone fails"""
    import zk_fhe_amd as zk
    _, g, _, _ = read_params(files["b"])
    g[5] = g[6]
    assert tampered(ctx, files, g=g, gl=ctx.g1_fft(g, inverse=True)) == zk.SRS_BAD_POWERS


def test_check_finds_a_wrong_lagrange_point(ctx, files):
    import zk_fhe_amd as zk
    _, _, gl, _ = read_params(files["b"])
    gl[3] = gl[4]
    assert tampered(ctx, files, gl=gl) == zk.SRS_BAD_LAGRANGE


def test_check_finds_a_wrong_g2(ctx, files):
    import zk_fhe_amd as zk
    g2, _ = files["g2"]
    assert tampered(ctx, files, g2=(g2, g2)) == zk.SRS_BAD_POWERS


def test_check_finds_a_wrong_generator(ctx, files):
    """every point doubled: still powers of s and still a Lagrange form, but of 2 G"""
    import zk_fhe_amd as zk
    _, g, gl, _ = read_params(files["b"])
    assert tampered(ctx, files, g=ctx.g1_add(g, g), gl=ctx.g1_add(gl, gl)) == zk.SRS_BAD_GENERATOR


def test_check_refuses_an_srs_without_g2(ctx, files):
    import zk_fhe_amd as zk
    _, g, gl, _ = read_params(files["b"])
    srs = zk.Srs.from_points(ctx, 9, g, gl)
    with pytest.raises(zk.ZkfheError, match="srs_check: the SRS has no G2 half"):
        srs.check(SEED)
    failed = ctypes.c_uint32()
    assert ctx.lib.zkfhe_srs_check(ctx.h, None, SEED, ctypes.byref(failed)) == -1
    assert ctx.lib.zkfhe_srs_check(ctx.h, srs.h, SEED, None) == -1
    assert ctx.lib.zkfhe_last_error(ctx.h).decode().startswith("srs_check:")
    srs.destroy()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def refused(ctx, prefix, call):
    """the call raises and the library's message starts with the prefix"""
    import zk_fhe_amd as zk
    with pytest.raises(zk.ZkfheError) as e:
        call()
    assert ("): " + prefix) in str(e.value), str(e.value)


def test_from_monomial_refusals(ctx, files):
    import zk_fhe_amd as zk
    _, g, _, _ = read_params(files["b"])
    g2, s_g2 = files["g2"]
    pre = "srs_from_monomial:"
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, g, g2, None))
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, g, None, s_g2))
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 2, g))
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 21, g))
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 10, g))           # 2^9 powers for k = 10
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, g[:511]))
    off_twist = ((g2[0][0], g2[0][1]), (g2[1][0] ^ 1, g2[1][1]))
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, g, off_twist, s_g2))
    bad = g.copy()
    bad[7, 4] ^= 1                                                         # a limb of one y: off the curve
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, bad))
    bad = g.copy()
    bad[7, :4] = np.uint64(0xffffffffffffffff)                             # x >= p
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, bad))
    bad = g.copy()
    bad[511] = 0                                                           # the identity among the powers
    refused(ctx, pre, lambda: zk.Srs.from_monomial(ctx, 9, bad))
    bad = np.concatenate([g, np.zeros((1, 8), dtype=np.uint64)])           # ... but not beyond them: a longer list is cut
    zk.Srs.from_monomial(ctx, 9, bad).destroy()
    # NULL arguments, straight at the C ABI
    lib = ctx.lib
    h = ctypes.c_void_p()
    assert lib.zkfhe_srs_from_monomial(ctx.h, 9, None, 512, None, None, ctypes.byref(h)) == -1
    assert lib.zkfhe_last_error(ctx.h).decode().startswith(pre)
    assert lib.zkfhe_srs_from_monomial(ctx.h, 9, g.ctypes.data_as(ctypes.c_void_p), 512, None, None, None) == -1
    assert lib.zkfhe_last_error(ctx.h).decode().startswith(pre)


def test_load_downsized_refusals(ctx, files, tmp_path):
    import zk_fhe_amd as zk
    pre = "srs_load_downsized:"
    blob = open(files["b"], "rb").read()
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, files["b"], 10))             # k_file = 9 < 10
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, files["b"], 2))
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, files["b"], 21))
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, str(tmp_path / "missing.srs"), 9))
    short = str(tmp_path / "short.srs")
    open(short, "wb").write(blob[:-9])
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, short, 9))
    framed = str(tmp_path / "framed.srs")
    open(framed, "wb").write((10).to_bytes(4, "little") + blob[4:])                   # the header promises 2^10 points
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, framed, 9))
    off = bytearray(blob)
    off[4 + 64 * 7 + 32] ^= 1                                                         # y of g[7]
    offp = str(tmp_path / "off.srs")
    open(offp, "wb").write(bytes(off))
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, offp, 9))
    ident = bytearray(blob)
    ident[4 + 64 * 3:4 + 64 * 4] = bytes(64)
    open(offp, "wb").write(bytes(ident))
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, offp, 9))
    g2off = bytearray(blob)
    g2off[-1 - 64] ^= 1                                                               # a coordinate of s G2
    open(offp, "wb").write(bytes(g2off))
    refused(ctx, pre, lambda: zk.Srs.load_downsized(ctx, offp, 9))
    # the file's g_lagrange is never read: garbage there changes nothing
    junk = bytearray(blob)
    junk[4 + 64 * 512:4 + 128 * 512] = bytes(64 * 512)
    open(offp, "wb").write(bytes(junk))
    out = str(tmp_path / "out.srs")
    srs = zk.Srs.load_downsized(ctx, offp, 9)
    srs.save(out)
    srs.destroy()
    assert same_file(out, files["b"])
    lib = ctx.lib
    h = ctypes.c_void_p()
    assert lib.zkfhe_srs_load_downsized(ctx.h, None, 9, ctypes.byref(h)) == -1
    assert lib.zkfhe_last_error(ctx.h).decode().startswith(pre)
    assert lib.zkfhe_srs_load_downsized(ctx.h, os.fsencode(files["b"]), 9, None) == -1


def test_argument_refusals_queue_no_device_work(ctx, files):
    """what the arguments alone decide is refused before the first command: the context's command counters do not move"""
    import zk_fhe_amd as zk
    _, g, _, _ = read_params(files["b"])
    g2, s_g2 = files["g2"]
    bad = g.copy()
    bad[7, 4] ^= 1
    before = ctx.last_proof_commands()
    for call in (lambda: zk.Srs.from_monomial(ctx, 9, g, g2, None), lambda: zk.Srs.from_monomial(ctx, 21, g), lambda: zk.Srs.from_monomial(ctx, 10, g),
                 lambda: zk.Srs.from_monomial(ctx, 9, bad), lambda: zk.Srs.load_downsized(ctx, files["b"], 10), lambda: zk.Srs.load_downsized(ctx, files["b"], 2)):
        with pytest.raises(zk.ZkfheError):
            call()
    assert ctx.last_proof_commands() == before
