"""`bfv -k <k> srs --from <params file of k_file >= k>`: the fifth command of the command-line driver, run as a subprocess in a
scratch directory (tests/test_cli.py covers the other four)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "zk-fhe_amd", "bfv")


def _run(cwd, *args, env=None):
    if not os.path.exists(EXE):
        pytest.skip("zk-fhe_amd/bfv is not built (python -c 'import __graft_entry__ as g; g.build()')")
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + list(args), cwd=str(cwd), capture_output=True, text=True, timeout=600, env=e)


def test_srs_needs_a_source(tmp_path):
    """host only: the argument check comes before the GPU is opened"""
    r = _run(tmp_path, "-k", "9", "srs")
    assert r.returncode == 2 and "--from" in r.stderr
    assert not os.path.exists(tmp_path / "params")


@pytest.mark.gpu
def test_srs_command_downsizes_checks_and_saves(tmp_path):
    import torch  # noqa: F401  (loads the ROCm runtime the extension links against first)
    import zk_fhe_amd as zk
    ctx = zk.Context(0)
    big, want = str(tmp_path / "k10.srs"), str(tmp_path / "k9.srs")
    s10, s9 = zk.Srs(ctx, 10), zk.Srs(ctx, 9)
    s10.save(big), s9.save(want)
    s10.destroy(), s9.destroy()
    ctx.close()
    out = tmp_path / "params" / "kzg_bn254_9.srs"
    r = _run(tmp_path, "-k", "9", "srs", "--from", big)
    assert r.returncode == 0 and "kzg_bn254_9.srs" in r.stdout, r.stdout + r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()
    # a second run refuses to overwrite
    stamp = os.stat(out).st_mtime_ns
    r = _run(tmp_path, "-k", "9", "srs", "--from", big)
    assert r.returncode != 0 and "not overwritten" in r.stderr and os.stat(out).st_mtime_ns == stamp
    # PARAMS_DIR is honoured, and a tampered source (g[5] := g[6]) is named and nothing is written
    blob = bytearray(open(big, "rb").read())
    blob[4 + 64 * 5:4 + 64 * 6] = blob[4 + 64 * 6:4 + 64 * 7]
    bad = str(tmp_path / "bad.srs")
    open(bad, "wb").write(bytes(blob))
    r = _run(tmp_path, "-k", "9", "srs", "--from", bad, env={"PARAMS_DIR": str(tmp_path / "other")})
    assert r.returncode != 0 and "powers" in r.stderr and "lagrange" not in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "other" / "kzg_bn254_9.srs")
    r = _run(tmp_path, "-k", "9", "srs", "--from", big, env={"PARAMS_DIR": str(tmp_path / "other")})
    assert r.returncode == 0 and open(tmp_path / "other" / "kzg_bn254_9.srs", "rb").read() == open(want, "rb").read()
    # a source that is too small
    r = _run(tmp_path, "-k", "10", "srs", "--from", want)
    assert r.returncode != 0 and "srs_load_downsized:" in r.stderr
