"""Filtering and detrending of traces -- ``Trace.filter`` / ``Trace.detrend`` of ObsPy, restated with the scipy calls ObsPy
itself makes (un-vendored, parity unpinned like the rest of the stream handling).  The reference's waveform inspection runs
``st.detrend("demean").detrend("linear")``, ``filter("highpass", freq=0.3)``, ``filter("bandpass", freqmin=1, freqmax=20)``
(volpick/data/utils.py:675-704), and SeisBench applies a model's ``filter_args`` / ``filter_kwargs`` to the stream inside
``annotate`` ahead of its resampling.

Host path: :func:`filter_array`, :func:`detrend_array` (scipy, float64, as ObsPy).  Device path: :func:`sos_filter_device`,
:func:`detrend_device` (``vp_sos_filter`` / ``vp_detrend``: float64 state, float32 result).  :func:`butter_sos` is the one
source of coefficients of both.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._device import device_backing, device_samples, release_scratch, sample_args, trace_in_place
from .resample import lowpass_sos

FILTER_TYPES = ("lowpass", "highpass", "bandpass", "bandstop")
DETREND_TYPES = {"demean": _lib.VP_DETREND_DEMEAN, "constant": _lib.VP_DETREND_DEMEAN, "linear": _lib.VP_DETREND_LINEAR,
                 "simple": _lib.VP_DETREND_SIMPLE}


def butter_sos(type, df, corners=4, freq=None, freqmin=None, freqmax=None):
    """Second-order sections (scipy's ``sos`` layout, float64) of ObsPy's Butterworth ``type`` filter at sampling rate ``df``,
    with ObsPy's Nyquist rules: a low-pass or band-stop corner above Nyquist is clamped with a warning, a band-pass whose
    upper corner reaches Nyquist becomes the high-pass of its lower corner with a warning, a lower corner above Nyquist is a
    ``ValueError``."""
    from scipy.signal import iirfilter, zpk2sos

    if type not in FILTER_TYPES:
        raise ValueError(f"filter type {type!r} is not one of {FILTER_TYPES}")
    fe = 0.5 * df
    if type in ("lowpass", "highpass"):
        if freq is None or freqmin is not None or freqmax is not None:
            raise TypeError(f"{type} takes freq=")
        if type == "lowpass":
            return lowpass_sos(freq, df, corners)
        f = freq / fe
        if f > 1:
            raise ValueError("Selected corner frequency is above Nyquist.")
        z, p, k = iirfilter(corners, f, btype="highpass", ftype="butter", output="zpk")
        return zpk2sos(z, p, k)
    if freqmin is None or freqmax is None or freq is not None:
        raise TypeError(f"{type} takes freqmin= and freqmax=")
    low, high = freqmin / fe, freqmax / fe
    if type == "bandpass":
        if high - 1.0 > -1e-6:
            warnings.warn(f"Selected high corner frequency ({freqmax}) of bandpass is at or above Nyquist ({fe}). "
                          "Applying a high-pass instead.")
            return butter_sos("highpass", df, corners, freq=freqmin)
    elif high > 1:
        high = 1.0
        warnings.warn("Selected high corner frequency is above Nyquist. Setting Nyquist as high corner.")
    if low > 1:
        raise ValueError("Selected low corner frequency is above Nyquist.")
    z, p, k = iirfilter(corners, [low, high], btype="band" if type == "bandpass" else "bandstop", ftype="butter", output="zpk")
    return zpk2sos(z, p, k)


def _not_masked(data, what):
    if np.ma.isMaskedArray(data):
        raise NotImplementedError(f"masked traces cannot be {what}; split the stream at its gaps first")


def filter_array(data, type, df, zerophase=False, **options):
    """``obspy.signal.filter.<type>(data, df=df, zerophase=zerophase, **options)``: float64 in scipy, float64 out."""
    from scipy.signal import sosfilt

    _not_masked(data, "filtered")
    sos = butter_sos(type, df, **options)
    x = np.asarray(data, dtype=np.float64)
    y = sosfilt(sos, x)
    return sosfilt(sos, y[::-1])[::-1] if zerophase else y


def detrend_array(data, type="simple"):
    """``Trace.detrend(type)`` for ``demean`` / ``constant``, ``linear`` and ``simple``: float64 out."""
    from scipy.signal import detrend

    _not_masked(data, "detrended")
    if type not in DETREND_TYPES:
        raise ValueError(f"detrend type {type!r} is not one of {sorted(DETREND_TYPES)}")
    x = np.array(data, dtype=np.float64)
    if type == "simple":
        if len(x) < 2:
            raise ValueError("detrend('simple') needs at least two samples")
        return x - (x[0] + np.arange(len(x)) * (x[-1] - x[0]) / float(len(x) - 1))
    if type == "linear" and len(x) < 2:
        raise ValueError("detrend('linear') needs at least two samples")
    return detrend(x, type="linear" if type == "linear" else "constant")


def sos_filter_device(x, sos, zerophase=False):
    """``sosfilt(sos, x)`` (with ``zerophase``: forward, then backward) on the GPU (``vp_sos_filter``): ``x`` is a 1-D CUDA
    tensor of int32, float32 or float64 samples, ``sos`` up to 4 sections in scipy's layout; returns a new float32 CUDA tensor
    of the same length.  float64 coefficients, state and intermediate, one rounding to float32 at the end.  Raises
    ``VolpickHipError`` where the library refuses (more than 4 sections, an unstable section, ``a0 != 1``): there is no silent
    host fallback inside this function."""
    import torch

    x = device_samples(x, "sos_filter_device")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    sos = np.ascontiguousarray(np.atleast_2d(np.asarray(sos, dtype=np.float64)))
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("sos_filter_device: sos must have six columns (scipy's sos layout)")
    _lib.check(_lib.load().vp_sos_filter(*sample_args(x), sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos),
                                         int(bool(zerophase)), C.c_void_p(out.data_ptr())), "vp_sos_filter")
    return out


def detrend_device(x, type="simple"):
    """:func:`detrend_array` on the GPU (``vp_detrend``): ``x`` is a 1-D CUDA tensor of int32, float32 or float64 samples;
    returns a new float32 CUDA tensor.  Sums in float64 in a fixed order.  Raises ``VolpickHipError`` where the library
    refuses (a line through fewer than two samples): no silent host fallback."""
    import torch

    if type not in DETREND_TYPES:
        raise ValueError(f"detrend type {type!r} is not one of {sorted(DETREND_TYPES)}")
    x = device_samples(x, "detrend_device")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().vp_detrend(*sample_args(x), DETREND_TYPES[type], C.c_void_p(out.data_ptr())), "vp_detrend")
    return out


def release_filter_scratch(device=0):
    """Free the scratch `sos_filter_device` and `detrend_device` keep per device between calls; returns the bytes freed."""
    return release_scratch("vp_sos_filter_release_scratch", device)


def filter_trace(tr, type, **options):
    """``tr.filter(type, **options)`` in place (``volpick_amd.Trace``): device-backed traces on the device, where they stay."""
    zerophase = bool(options.pop("zerophase", False))
    df = float(tr.stats.sampling_rate)
    return trace_in_place(tr, "filtering", lambda dev: sos_filter_device(dev, butter_sos(type, df, **options), zerophase),
                          lambda a: filter_array(a, type, df, zerophase=zerophase, **options))


def detrend_trace(tr, type="simple"):
    """``tr.detrend(type)`` in place (``volpick_amd.Trace``): device-backed traces on the device, where they stay."""
    if type not in DETREND_TYPES:
        raise ValueError(f"detrend type {type!r} is not one of {sorted(DETREND_TYPES)}")
    return trace_in_place(tr, "detrending", lambda dev: detrend_device(dev, type), lambda a: detrend_array(a, type))


def filtered_copy(tr, type, **options):
    """A filtered copy of ``tr``; the caller's trace, device-backed or not, is left alone.  A device trace's copy is built on
    the device directly (``Trace.copy()`` would go through the host)."""
    from .stream import Trace

    dev = device_backing(tr)
    if isinstance(tr, Trace) and dev is not None:
        out = Trace(header=tr.stats.copy(), device_data=dev)  # shares the samples: the filter writes a new tensor
    else:
        out = tr.copy()
    if isinstance(out, Trace):
        return filter_trace(out, type, **options)
    return out.filter(type, **options)  # an ObsPy trace filters itself
