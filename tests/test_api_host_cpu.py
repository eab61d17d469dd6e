"""The host logic of the C ABI that needs no GPU (volpick_amd/csrc/api_host.h): WindowPlan, ScanLayout and collect_rows against
the code they replaced in api.hip, kept word for word in tests/api_host_check.cpp, and against the oracle's window rule.  Built
with the host compiler alone, under AddressSanitizer and UndefinedBehaviorSanitizer where their runtime links."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_window_plan_scan_layout_and_collect_equal_the_code_they_replaced(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/llvm/bin/clang++")
    exe = tmp_path / "api_host_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-I", str(ROOT / "volpick_amd" / "csrc"),
           str(ROOT / "tests" / "api_host_check.cpp"), "-o", str(exe)]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + sanitize, capture_output=True).returncode != 0:  # no sanitizer runtime for this compiler
        print("sanitizer build failed; building without")
        subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.count("identical") == 3 and "DIFFERENT" not in r.stdout
