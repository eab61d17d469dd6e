"""The three-piece bfloat16 packers of the ResCNN and decoder-tail planners (volpick_amd/csrc/bf16_pack.cpp) go through
bf16_split3; tests/bf16_pack_check.cpp holds the inline splits they replaced and compares the packed bytes.  Host code
only: built with the host compiler, no HIP runtime, no GPU."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_packed_operands_equal_the_inline_splits_byte_for_byte(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/llvm/bin/clang++")
    exe = tmp_path / "bf16_pack_check"
    csrc = ROOT / "volpick_amd" / "csrc"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", str(csrc), str(ROOT / "tests" / "bf16_pack_check.cpp"),
                    str(csrc / "bf16_pack.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("identical") == 4 and "DIFFERENT" not in r.stdout
