"""vp_mseed_scan from eight std::threads under ThreadSanitizer: tests/mseed_scan_threads.cpp, a program with a main of its own,
compiled together with volpick_amd/csrc/mseed.hip by hipcc with the sanitizer on the host side only.  It scans the file this
test writes (miniSEED 2 and miniSEED 3 records mixed), with no scan before its threads start, compares every thread's record
table and checks that each thread reads its own refusal text.  No GPU, nothing loaded into python."""
import os
import shutil
import subprocess
from pathlib import Path

from tests.mseed_util import mixed_file_bytes

ROOT = Path(__file__).resolve().parents[1]


def test_scan_threads_under_thread_sanitizer(tmp_path):
    (tmp_path / "mixed.mseed").write_bytes(mixed_file_bytes())
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "volpick_amd" / "csrc"
    exe = tmp_path / "mseed_scan_threads"
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-pthread", "-I", str(csrc), "-I", str(ROOT / "include"),
           "-x", "hip", str(csrc / "mseed.hip"), "-x", "c++", str(ROOT / "tests" / "mseed_scan_threads.cpp"), "-o", str(exe)]
    sanitize = ["-Xarch_host", "-fsanitize=thread"]
    built = subprocess.run(cmd + sanitize, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:  # no ThreadSanitizer runtime for this compiler
        print("sanitizer build failed; building without\n" + built.stderr[-2000:])
        subprocess.run(cmd, check=True)
    print(f"compiler: {hipcc}; ThreadSanitizer linked: {'yes' if sanitized else 'NO'}")
    r = subprocess.run([str(exe), str(tmp_path / "mixed.mseed")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.count("identical") == 1 and "DIFFERENT" not in r.stdout
    assert r.stdout.startswith("8 threads, ")
