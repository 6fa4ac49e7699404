"""The committed zk-fhe_amd/csrc/mont29_tied.inc (the nine-limb Montgomery products as inline assembly) is what
tools/gen_tied_products.py writes: a hand edit of the generated file, or a change of the generator without regenerating, fails here."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_tied_products_are_what_the_generator_writes(tmp_path):
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tied_products.py"), "--out-dir", str(tmp_path)], check=True)
    written = (tmp_path / "mont29_tied.inc").read_bytes()
    committed = open(os.path.join(ROOT, "zk-fhe_amd", "csrc", "mont29_tied.inc"), "rb").read()
    assert written == committed
