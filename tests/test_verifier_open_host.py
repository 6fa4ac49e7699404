"""The verifier's proof reader and opening (host/proof_reader.hpp, host/opening.cpp) on hostile bytes, on the CPU alone
(tests/native/verifier_open_check.cpp)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "zk-fhe_amd", "host")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_opening_on_hostile_bytes(tmp_path, sanitize):
    """The oracle-made toy proof (41 instances, 278 words): accepted; each of its 278 prefixes at a word boundary is "proof truncated"
    and one extra word "trailing bytes in proof", each opened from a buffer of exactly its length; opening from the transcript state
    after digest | pk0 | pk1 (16 instances), and from pre-decoded points, equals opening from the start; x >= q, an x with no root and
    an identity with a stray byte in commitment 1 are refused with the same text whether decoded on the host or ahead of the replay.
    Built plain and under the address and undefined-behaviour sanitizers; the program is stand-alone: nothing is preloaded.
    The program runs about 1 s plain and 1.5 s sanitized on 8 CPUs; compiling its five units (10 s, 20 s sanitized) is most of the test."""
    from tests.test_host_verifier import make
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++ (the host headers use clang's carry builtins)")
    vkb, inst, proof = make("poseidon")
    assert len(inst) == 41 and len(proof) == 278 * 32
    for name, data in (("vk", vkb), ("inst", b"".join(int(v).to_bytes(32, "little") for v in inst)), ("proof", proof)):
        (tmp_path / name).write_bytes(data)
    exe = str(tmp_path / "verifier_open_check")
    flags = ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    units = [os.path.join(HERE, "native", "verifier_open_check.cpp")] + [os.path.join(HOST, f) for f in ("opening.cpp", "host_g2.cpp", "poseidon_ifma.cpp", "poseidon_x8.cpp")]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", "-I", HOST, *units, "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe, str(tmp_path / "vk"), str(tmp_path / "inst"), str(tmp_path / "proof"), "16"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
