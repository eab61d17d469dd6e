"""What the device paths of the trace operations (resample.py, signal.py, io.py) share: which tensors the library takes as
samples, the release call of an operation's per-device scratch, and the step "on the device, or said aloud why not"."""
from __future__ import annotations

import ctypes as C
import warnings

from . import _lib

SAMPLE_KINDS = {"torch.int32": _lib.VP_SAMPLES_INT32, "torch.float32": _lib.VP_SAMPLES_FLOAT32,
                "torch.float64": _lib.VP_SAMPLES_FLOAT64}


def device_samples(x, who):
    """``x`` contiguous, if it is what the library's ``in_dev`` / ``in_kind`` arguments take; ``who`` names the caller."""
    import torch

    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 1 and str(x.dtype) in SAMPLE_KINDS):
        raise TypeError(f"{who}: need a 1-D CUDA tensor of int32, float32 or float64 samples")
    return x.contiguous()


def release_scratch(symbol, device):
    """``symbol(device, &bytes_freed)`` of the library (a ``vp_*_release_scratch``); returns the bytes freed."""
    freed = C.c_size_t(0)
    _lib.check(getattr(_lib.load(), symbol)(int(device), C.byref(freed)), symbol)
    return int(freed.value)


def try_on_device(trace_id, what, run, host_what):
    """``run()``; where the library refuses (``VolpickHipError``), a warning in the caller's name and ``None``: the caller
    then takes its host path."""
    try:
        return run()
    except _lib.VolpickHipError as e:
        warnings.warn(f"{trace_id}: {what} on the device refused ({e}); {host_what} on the host", stacklevel=2)
        return None
