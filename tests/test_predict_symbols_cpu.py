"""CPU: the prediction entry points are declared in the header, exported by the library and bound in _lib.py with the
header's argument counts; the record layouts of the header, _lib.py and evaluate.py agree."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from volpick_amd import _lib, evaluate

HEADER = (Path(__file__).resolve().parents[1] / "include" / "volpick_hip.h").read_text()
NAMES = ["vp_predict_windows", "vp_predict_begin", "vp_predict_bank", "vp_predict_end"]


def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        m = re.search(r"^int " + name + r"\(([^;]*)\);", HEADER, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported"


def test_constants_and_record_layout():
    assert re.search(r"enum \{ VP_DET_ONE_MINUS_NOISE = 0, VP_DET_ROW = 1 \};", HEADER)
    assert (_lib.VP_DET_ONE_MINUS_NOISE, _lib.VP_DET_ROW) == (0, 1)
    assert "float det, p_max, s_max;\n  int32_t p_arg, s_arg;\n} vp_predict_record;" in HEADER
    assert C.sizeof(_lib.VpPredictRecord) == 20 == evaluate.RECORD.itemsize
    assert [f[0] for f in _lib.VpPredictRecord._fields_] == list(evaluate.RECORD.names)
    assert [evaluate.RECORD.fields[n][1] for n in evaluate.RECORD.names] == [0, 4, 8, 12, 16]


def test_null_arguments_are_refused_without_a_device(lib):
    rec = np.zeros(1, evaluate.RECORD)
    assert lib.vp_predict_windows(None, None, 0, 1, 3, 0, 1, 2, 0, None, None, rec.ctypes.data_as(C.c_void_p)) == -1
    assert lib.vp_predict_begin(None) == -1 and lib.vp_predict_end(None, None, 0, None) == -1
    assert lib.vp_predict_bank(None, None, None, None, None, 1, 0, 0, 1, 2, None) == -1
    assert b"null" in lib.vp_last_error()
