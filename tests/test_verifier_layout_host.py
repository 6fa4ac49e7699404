"""host/shplonk.hpp on the CPU: a proof's word count by the one opening layout (tests/native/verifier_layout_check.cpp)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "zk-fhe_amd", "host")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_verifier_layout(tmp_path, sanitize):
    """Toy, pinned k = 13 and the widest shape the vk parser admits: proof_words is the earlier closed formula, and the layout's
    evaluation words are the rotation counts of every item but H.  For the toy configuration of the oracle the printed count is
    the length of an oracle-made proof under both transcripts.  Built plain and under the address and undefined-behaviour
    sanitizers; the program is stand-alone: nothing is preloaded."""
    from oracle import circuit_ref as C
    from oracle import halo2_ref as H
    from tests.test_host_verifier import make
    from tests.test_proof_oracle import synth_input
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++")
    exe = str(tmp_path / "verifier_layout_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", HOST, os.path.join(HERE, "native", "verifier_layout_check.cpp"), "-o", exe], check=True)
    prm = C.BfvParams(N=8)
    cfg = H.auto_config(9, 9, H.BfvCircuit(synth_input(8, prm.Q, prm.T, prm.B, 1), prm))
    args = [cfg.k, cfg.n_gate0, cfg.n_gate1, cfg.n_lookup, cfg.n_rlc, cfg.unusable_rows]
    out = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    words = int(re.search(r"proof_words (\d+)", out.stdout).group(1))
    for kind in ("poseidon", "blake2b"):
        proof = _toy_proof(kind, make)
        assert len(proof) % 32 == 0 and words == len(proof) // 32


_PROOFS = {}


def _toy_proof(kind, make):
    """the oracle-made toy proof of tests/test_host_verifier.py, made once per transcript"""
    if kind not in _PROOFS:
        _PROOFS[kind] = make(kind)[2]
    return _PROOFS[kind]
