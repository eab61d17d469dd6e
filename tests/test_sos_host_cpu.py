"""The host checks the trace operations share (volpick_amd/csrc/sos_host.h: check_sample_kind, load_sos, warmup_length) against
the two make_plan bodies and the warmup_length they replaced, kept word for word in tests/sos_host_check.cpp.  Built with the
host compiler alone, under AddressSanitizer and UndefinedBehaviorSanitizer where their runtime links; the coefficient tables
come from the package's own butter_sos / lowpass_sos."""
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np

from volpick_amd.resample import lowpass_sos
from volpick_amd.signal import butter_sos

ROOT = Path(__file__).resolve().parents[1]
HALO = 1024  # resample.hip: DHALO
VP_OK, VP_ERR_UNSUPPORTED = 0, -4


def decimate_code(sos):
    """What decimation answers to a stable table: its warm-up (r^W <= 2^-40, plus two samples per section) against the halo,
    with the pole radius from numpy's roots, not from the code under test."""
    r = max(abs(z) for row in sos for z in np.roots(row[3:]))
    assert r < 1.0
    return VP_ERR_UNSUPPORTED if math.ceil(40.0 * math.log(2.0) / -math.log(r)) + 2 * len(sos) > HALO else VP_OK


def tables():
    out = {}
    for ns in (1, 2, 3, 4):  # 2 ns corners give ns sections for low- and high-pass, ns corners for the two band filters
        out[f"lowpass_{ns}"] = butter_sos("lowpass", 100.0, corners=2 * ns, freq=10.0)
        out[f"highpass_{ns}"] = butter_sos("highpass", 100.0, corners=2 * ns, freq=0.3)
        out[f"bandpass_{ns}"] = butter_sos("bandpass", 100.0, corners=ns, freqmin=1.0, freqmax=20.0)
        out[f"bandstop_{ns}"] = butter_sos("bandstop", 100.0, corners=ns, freqmin=1.0, freqmax=20.0)
        assert all(len(out[f"{k}_{ns}"]) == ns for k in ("lowpass", "highpass", "bandpass", "bandstop"))
    out["long_warmup_lowpass_50_25000"] = lowpass_sos(50.0, 25000.0)
    return out


def test_load_sos_and_warmup_equal_the_code_they_replaced(tmp_path):
    tabs = tables()
    assert decimate_code(tabs["long_warmup_lowpass_50_25000"]) == VP_ERR_UNSUPPORTED
    assert decimate_code(tabs["lowpass_4"]) == VP_OK
    lines = []
    for name, sos in tabs.items():
        sos = np.asarray(sos, dtype=np.float64)
        lines.append(f"{name} {len(sos)} {decimate_code(sos)}")
        lines += [" ".join(float(v).hex() for v in row) for row in sos]
    (tmp_path / "tables.txt").write_text("\n".join(lines) + "\n")

    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/llvm/bin/clang++")
    exe = tmp_path / "sos_host_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-I", str(ROOT / "volpick_amd" / "csrc"),
           str(ROOT / "tests" / "sos_host_check.cpp"), "-o", str(exe)]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + sanitize, capture_output=True).returncode != 0:  # no sanitizer runtime for this compiler
        print("sanitizer build failed; building without")
        subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe), str(tmp_path / "tables.txt")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.count("identical") == 1 and "DIFFERENT" not in r.stdout
    assert r.stdout.startswith(f"{len(tabs)} tables, ")
