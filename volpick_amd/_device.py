"""What the device paths of the trace operations (io.py, stream.py, signal.py, resample.py, trigger.py, spectrogram.py,
attributes.py, convert.py) share.

* A trace's backing: :func:`device_backing` / :func:`trace_samples` read it (on ``volpick_amd.Trace``, ObsPy traces and
  anything else), :func:`replace_samples` swaps it, :func:`upload_samples` is the one rule by which a host array becomes one.
  No other module touches ``Trace._dev`` / ``Trace._data`` of a trace it has not just built.
* A call into the library: :func:`device_samples` checks the tensor, :func:`sample_args` gives the call's leading arguments
  for entry points that work on the null stream, :func:`stream_handle` the stream argument of those that take one,
  :func:`release_scratch` frees an operation's per-device scratch.
* The step "on the device, or said aloud why not": :func:`try_on_device`; :func:`trace_on_device` for one trace;
  :func:`trace_in_place` with the host path and the swap of the backing behind it.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib

SAMPLE_KINDS = {"torch.int32": _lib.VP_SAMPLES_INT32, "torch.float32": _lib.VP_SAMPLES_FLOAT32,
                "torch.float64": _lib.VP_SAMPLES_FLOAT64}


def is_cuda(a):
    """Whether ``a`` is a CUDA tensor, without importing torch for a numpy array."""
    return type(a).__module__.startswith("torch") and getattr(a, "is_cuda", False)


def device_samples(x, who, dims=(1,)):
    """``x`` contiguous, if it is what the library's ``in_dev`` / ``in_kind`` arguments take; ``who`` names the caller."""
    if not (is_cuda(x) and x.dim() in dims and str(x.dtype) in SAMPLE_KINDS):
        raise TypeError(f"{who}: need a {' or '.join(f'{d}-D' for d in dims)} CUDA tensor of int32, float32 or float64 samples")
    return x.contiguous()


def sample_args(x):
    """``(device index, pointer, kind, n)`` -- how every per-trace entry point of the library begins -- of checked samples
    ``x`` (``n``: the length of a series).  The library works on the null stream, so torch's current stream on that device is
    synchronised first: ``x`` is complete before the library starts."""
    import torch

    torch.cuda.current_stream(x.device).synchronize()
    return x.device.index, C.c_void_p(x.data_ptr()), SAMPLE_KINDS[str(x.dtype)], int(x.shape[-1])


def stream_handle(device):
    """torch's current stream on ``device`` (an index or a ``torch.device``) as the library's ``stream`` argument."""
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def release_scratch(symbol, device):
    """``symbol(device, &bytes_freed)`` of the library (a ``vp_*_release_scratch``); returns the bytes freed."""
    freed = C.c_size_t(0)
    _lib.check(getattr(_lib.load(), symbol)(int(device), C.byref(freed)), symbol)
    return int(freed.value)


def device_backing(tr):
    """The device tensor behind a trace, whatever its dtype; ``None`` for a host trace, an ObsPy trace, anything else."""
    return getattr(tr, "_dev", None)


def trace_samples(tr):
    """The device tensor behind a trace if it is of a kind the library takes (int32, float32, float64), else ``None``."""
    dev = device_backing(tr)
    return dev if dev is not None and str(dev.dtype) in SAMPLE_KINDS else None


def replace_samples(tr, dev):
    """``tr`` (a ``volpick_amd.Trace``) is backed by the device tensor ``dev`` from now on: no host copy, ``npts`` its length."""
    tr._dev, tr._data = dev, None
    tr.stats["npts"] = int(dev.shape[0])


def upload_samples(a, device, refusal):
    """A host array as a tensor on ``device`` (a ``torch.device``), in its own dtype if that is int32, float32 or float64, as
    float32 otherwise.  A masked array is refused with the caller's sentence ``refusal``."""
    import torch

    if np.ma.isMaskedArray(a):
        raise NotImplementedError(f"{refusal}; split the stream at its gaps first")
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.dtype(np.int32), np.dtype(np.float32), np.dtype(np.float64)):
        a = a.astype(np.float32)
    return torch.from_numpy(a).to(device)


def try_on_device(trace_id, what, run, host_what):
    """``run()``; where the library refuses (``VolpickHipError``), a warning in the caller's name and ``None``: the caller
    then takes its host path."""
    try:
        return run()
    except _lib.VolpickHipError as e:
        warnings.warn(f"{trace_id}: {what} on the device refused ({e}); {host_what} on the host", stacklevel=2)
        return None


def trace_on_device(tr, what, host_what, run):
    """``run(samples)`` under :func:`try_on_device` if ``tr`` holds device samples: the new device tensor, or ``None`` where
    the trace holds none or the library refused."""
    dev = trace_samples(tr)
    return None if dev is None else try_on_device(tr.id, what, lambda: run(dev), host_what)


def trace_in_place(tr, what, run, host):
    """``tr`` processed in place: on the device if it lives there (``run``: device tensor -> new device tensor), on the host
    otherwise or where the library refuses (``host``: ndarray -> ndarray).  Returns ``tr``."""
    y = trace_on_device(tr, what, what, run)
    if y is not None:
        replace_samples(tr, y)
    else:
        tr.data = host(tr.data)
    return tr
