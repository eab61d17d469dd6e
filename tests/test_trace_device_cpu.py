"""What the device paths of the trace operations share on the Python side (volpick_amd/_device.py), as far as it can be checked
without a GPU: which tensors are refused, in whose name, and that the kind and type tables are the library's constants."""
import re
from pathlib import Path

import pytest
import torch

from volpick_amd import _device, _lib, resample, signal

HEADER = (Path(__file__).resolve().parents[1] / "include" / "volpick_hip.h").read_text()

NOT_SAMPLES = {
    "a CPU tensor": torch.zeros(8, dtype=torch.float32),
    "a 2-D tensor": torch.zeros(2, 8, dtype=torch.float32),
    "an int64 tensor": torch.zeros(8, dtype=torch.int64),
}


@pytest.mark.parametrize("what", sorted(NOT_SAMPLES))
def test_device_samples_refuses_in_the_callers_name(what):
    x = NOT_SAMPLES[what]
    with pytest.raises(TypeError, match=r"^some_caller: need a 1-D CUDA tensor of int32, float32 or float64 samples$"):
        _device.device_samples(x, "some_caller")
    calls = {
        "decimate_device": lambda: resample.decimate_device(x, 200.0, 100.0),
        "fourier_device": lambda: resample.fourier_device(x, 250.0, 100.0),
        "sos_filter_device": lambda: signal.sos_filter_device(x, signal.butter_sos("lowpass", 100.0, freq=10.0)),
        "detrend_device": lambda: signal.detrend_device(x, "linear"),
    }
    for who, call in calls.items():
        with pytest.raises(TypeError, match=rf"^{who}: need a 1-D CUDA tensor of int32, float32 or float64 samples$"):
            call()


def header_constant(name):
    return int(re.search(rf"\b{name} = (-?\d+)", HEADER).group(1))


def test_kind_and_type_tables_are_the_librarys_constants():
    assert _device.SAMPLE_KINDS == {"torch.int32": _lib.VP_SAMPLES_INT32, "torch.float32": _lib.VP_SAMPLES_FLOAT32,
                                    "torch.float64": _lib.VP_SAMPLES_FLOAT64}
    assert signal.DETREND_TYPES == {"demean": _lib.VP_DETREND_DEMEAN, "constant": _lib.VP_DETREND_DEMEAN,
                                    "linear": _lib.VP_DETREND_LINEAR, "simple": _lib.VP_DETREND_SIMPLE}
    for name in ("VP_SAMPLES_INT32", "VP_SAMPLES_FLOAT32", "VP_SAMPLES_FLOAT64", "VP_DETREND_DEMEAN", "VP_DETREND_LINEAR",
                 "VP_DETREND_SIMPLE"):
        assert getattr(_lib, name) == header_constant(name), name
    assert [str(getattr(torch, k.split(".")[1])) for k in _device.SAMPLE_KINDS] == list(_device.SAMPLE_KINDS)
