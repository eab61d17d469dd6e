"""CPU: the sweep entry points are declared in the header, exported by the library and bound in _lib.py with the header's
argument counts; the limits of the header, the kernel and evaluate.py agree; null arguments are refused without a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import volpick_amd
from volpick_amd import _lib, evaluate

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "volpick_hip.h").read_text()
NAMES = ["vp_sweep_windows", "vp_sweep_begin", "vp_sweep_bank", "vp_sweep_end"]


def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        m = re.search(r"^int " + name + r"\(([^;]*)\);", HEADER, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported"


def test_limits_agree_and_the_functions_are_exported():
    sweep_h = (ROOT / "volpick_amd" / "csrc" / "sweep.h").read_text()
    assert re.search(r"#define VP_SWEEP_MAX_T 6400\b", HEADER) and "SW_MAX_T == VP_SWEEP_MAX_T" in sweep_h
    assert re.search(r"SW_MAX_NT = 32;", sweep_h) and evaluate.SWEEP_MAX_THRESHOLDS == 32
    assert re.search(r"SW_MAX_K = 64;", sweep_h) and evaluate.SWEEP_MAX_PICKS == 64
    assert evaluate.SWEEP_COMPARE_DTYPE is np.float32 and evaluate.SWEEP_OFF_FRACTION == 2
    for name in ("sweep_windows", "sweep_bank", "eval_task0", "task0_truth", "task0_counts", "task0_residuals",
                 "task0_metrics", "task0_tnr", "opt_prob_metrics"):
        assert getattr(volpick_amd, name) is getattr(evaluate, name)


def test_null_arguments_are_refused_without_a_device(lib):
    thr = np.array([0.3], np.float32)
    count, peak = np.full(2, -77, np.int32), np.full(16, -77, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vp_sweep_windows(None, None, 0, 1, 3, 1, 2, None, None, p(thr), p(thr), 1, 8, p(count), p(peak), None) == -1
    assert b"null" in lib.vp_last_error()
    assert lib.vp_sweep_begin(None, p(thr), p(thr), 1, 8, 0) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_sweep_bank(None, None, None, None, None, 1, 0, 1, 2, None) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_sweep_end(None, p(count), p(peak), None, 1, None) == -1 and b"null" in lib.vp_last_error()
    assert (count == -77).all() and (peak == -77).all()
