"""Sampling-rate conversion of the traces handed to annotate()/classify() — host-side stream preparation, as in the
reference's path: SeisBench ``WaveformModel.annotate`` resamples every trace whose rate differs from the model's before
it groups them (``seisbench_requirement >= 0.4.0``, Final_models/**/volpick.json.v1:8; un-vendored, restated here from the
published SeisBench / ObsPy algorithm — parity unpinned, like the rest of the stream handling):

    rate % model_rate == 0 :  trace.filter("lowpass", freq=model_rate / 2, zerophase=True)
                              trace.decimate(rate // model_rate, no_filter=True)
    otherwise              :  trace.resample(model_rate, no_filter=True)       (ObsPy: Fourier method, Hann window)

ObsPy's building blocks, restated with the scipy calls ObsPy itself makes:
  * ``obspy.signal.filter.lowpass``: 4-corner Butterworth as second-order sections, forward pass + time-reversed pass;
  * ``Trace.decimate(no_filter=True)``: every factor-th sample;
  * ``Trace.resample(window="hann")``: real FFT, spectrum multiplied by a Hann window centred on DC, real and imaginary
    parts linearly interpolated onto the frequency grid of the new length, inverse real FFT, amplitude rescaled.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._device import device_samples, release_scratch, replace_samples, sample_args, trace_on_device


def lowpass_sos(freq, df, corners=4):
    """Second-order sections (scipy's ``sos`` layout, float64) of ObsPy's Butterworth low-pass with corner ``freq`` at
    sampling rate ``df``: the one source of filter coefficients of the host path and the device path."""
    from scipy.signal import iirfilter, zpk2sos

    fe = 0.5 * df
    f = freq / fe
    if f > 1:
        f = 1.0
        warnings.warn("Selected corner frequency is above Nyquist. Setting Nyquist as high corner.")
    z, p, k = iirfilter(corners, f, btype="lowpass", ftype="butter", output="zpk")
    return zpk2sos(z, p, k)


def lowpass_zerophase(data, freq, df, corners=4):
    from scipy.signal import sosfilt

    sos = lowpass_sos(freq, df, corners)
    firstpass = sosfilt(sos, data)
    return sosfilt(sos, firstpass[::-1])[::-1]


def resample_fourier(data, rate_in, rate_out, window="hann"):
    from scipy.fftpack import irfft, rfft
    from scipy.signal import get_window

    data = np.asarray(data)
    npts = len(data)
    factor = rate_in / float(rate_out)
    x = rfft(data if data.dtype.kind == "f" else data.astype(np.float64))
    x = np.insert(x, 1, x.dtype.type(0))
    if npts % 2 == 0:
        x = np.append(x, [0])
    x_r = x[::2]
    x_i = x[1::2]
    if window is not None:
        large_w = np.fft.ifftshift(get_window(window, npts))
        x_r *= large_w[: npts // 2 + 1]
        x_i *= large_w[: npts // 2 + 1]
    num = int(npts / factor)
    df = 1.0 / (npts * (1.0 / rate_in))
    d_large_f = 1.0 / num * rate_out
    f = df * np.arange(0, npts // 2 + 1, dtype=np.int32)
    n_large_f = num // 2 + 1
    large_f = d_large_f * np.arange(0, n_large_f, dtype=np.int32)
    large_y = np.zeros(2 * n_large_f)
    large_y[::2] = np.interp(large_f, f, x_r)
    large_y[1::2] = np.interp(large_f, f, x_i)
    large_y = np.delete(large_y, 1)
    if num % 2 == 0:
        large_y = np.delete(large_y, -1)
    return irfft(large_y) * (float(num) / float(npts))


def resample_array(data, rate_in, rate_out):
    """One trace's samples at ``rate_in`` -> samples at ``rate_out`` by the SeisBench rule (module docstring)."""
    if np.ma.isMaskedArray(data):
        raise NotImplementedError("masked traces cannot be resampled; split the stream at its gaps first")
    rate_in, rate_out = float(rate_in), float(rate_out)
    if rate_in == rate_out:
        return np.asarray(data)
    if rate_in % rate_out == 0:
        y = lowpass_zerophase(np.asarray(data, dtype=np.float64), rate_out * 0.5, rate_in)
        return np.ascontiguousarray(y[:: int(rate_in / rate_out)])
    return resample_fourier(data, rate_in, rate_out)


def decimate_device(x, rate_in, rate_out):
    """The integer-ratio branch of :func:`resample_array` on the GPU (``vp_decimate_lowpass``): ``x`` is a 1-D CUDA tensor
    of int32, float32 or float64 samples at ``rate_in``, an integer multiple (>= 2) of ``rate_out``; returns a float32 CUDA
    tensor of ``ceil(len(x) / k)`` samples.  Same coefficients as the host path (:func:`lowpass_sos`), float64 state and
    intermediate, one rounding to float32 at the end.  Raises ``VolpickHipError`` where the library refuses (a factor whose
    warm-up does not fit the kernel's tile): there is no silent host fallback inside this function."""
    import torch

    rate_in, rate_out = float(rate_in), float(rate_out)
    if not (rate_in % rate_out == 0 and rate_in > rate_out):
        raise ValueError(f"decimate_device: {rate_in} Hz is not an integer multiple (>= 2) of {rate_out} Hz")
    x = device_samples(x, "decimate_device")
    k = int(rate_in / rate_out)
    n = int(x.shape[0])
    out = torch.empty((n + k - 1) // k, dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    sos = np.ascontiguousarray(lowpass_sos(rate_out * 0.5, rate_in), dtype=np.float64)
    _lib.check(_lib.load().vp_decimate_lowpass(*sample_args(x), sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos), k,
                                               C.c_void_p(out.data_ptr()), out.shape[0]), "vp_decimate_lowpass")
    return out


def release_decimate_scratch(device=0):
    """Free the float64 scratch `decimate_device` keeps per device between calls; returns the bytes freed."""
    return release_scratch("vp_decimate_release_scratch", device)


def fourier_args(n, rate_in, rate_out):
    """``num``, ``df`` and ``d_large_f`` with exactly the expressions of :func:`resample_fourier`: the device path is handed
    the host path's float64 values, not a restatement of them."""
    factor = rate_in / float(rate_out)
    num = int(n / factor)
    df = 1.0 / (n * (1.0 / rate_in))
    d_large_f = 1.0 / num * rate_out if num >= 1 else float("nan")
    return num, df, d_large_f


def fourier_device(x, rate_in, rate_out):
    """The other branch of :func:`resample_array` on the GPU (``vp_resample_fourier``), :func:`decimate_device`'s twin: ``x``
    is a 1-D CUDA tensor of int32, float32 or float64 samples at ``rate_in``, no integer multiple of ``rate_out``; returns a
    float32 CUDA tensor of ``int(len(x) / (rate_in / rate_out))`` samples.  :func:`resample_fourier` in float64 on the device
    (Bluestein chirp-z transforms, so any length costs the same), one rounding to float32 at the end.

    float32 samples are widened and transformed in float64.  The host path transforms float32 input in single precision
    (scipy.fftpack keeps the dtype), so for such traces the device answer is the more accurate of the two and the host one
    differs from it by single-precision rounding noise.

    Raises ``ValueError`` for equal rates, an integer ratio (the other branch) and a trace too short to give one output
    sample; ``VolpickHipError`` where the library refuses (a trace beyond its largest transform, no memory for the scratch):
    there is no silent host fallback inside this function."""
    import torch

    rate_in, rate_out = float(rate_in), float(rate_out)
    if rate_in == rate_out:
        raise ValueError(f"fourier_device: the trace already is at {rate_out} Hz")
    if rate_in % rate_out == 0:
        raise ValueError(f"fourier_device: {rate_in} Hz is an integer multiple of {rate_out} Hz: that is decimate_device's branch")
    x = device_samples(x, "fourier_device")
    n = int(x.shape[0])
    num, df, d_large_f = fourier_args(n, rate_in, rate_out) if n else (0, 0.0, 0.0)
    if num < 1:
        raise ValueError(f"fourier_device: {n} samples at {rate_in} Hz give no sample at {rate_out} Hz")
    out = torch.empty(num, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().vp_resample_fourier(*sample_args(x), rate_in, rate_out, num, df, d_large_f,
                                               C.c_void_p(out.data_ptr()), num), "vp_resample_fourier")
    return out


def release_fourier_scratch(device=0):
    """Free the FFT buffers `fourier_device` keeps per device between calls; returns the bytes freed."""
    return release_scratch("vp_resample_release_scratch", device)


def resample_trace(tr, rate_out, copy=True, fourier_on_device=False):
    """A trace at ``rate_out``: the trace itself if it already is, a resampled copy (or, with ``copy=False``, the trace
    resampled in place, as upstream does) otherwise.  Works on ``volpick_amd.Trace`` and on ObsPy traces.

    A device-backed ``volpick_amd.Trace`` whose rate is an integer multiple of ``rate_out`` is decimated on the GPU
    (:func:`decimate_device`) and stays there: no host copy of it is made.  With ``fourier_on_device=True`` (what
    ``annotate`` / ``classify`` pass) a device-backed trace at any other rate is resampled there too
    (:func:`fourier_device`; for float32 samples that is the float64 answer, where the host path computes in single
    precision).  Every other case -- host traces, and device-backed ones on the Fourier branch by default -- takes the host
    path."""
    rate_in = float(tr.stats.sampling_rate)
    if abs(rate_in - rate_out) <= 1e-6:
        return tr
    # refused: a factor beyond the kernel's tile, a trace beyond the largest FFT: said aloud, then the host path below
    y = None
    if rate_in % float(rate_out) == 0 and rate_in > rate_out:
        y = trace_on_device(tr, "decimation", "resampling", lambda dev: decimate_device(dev, rate_in, rate_out))
    elif fourier_on_device:
        y = trace_on_device(tr, "Fourier resampling", "resampling", lambda dev: fourier_device(dev, rate_in, float(rate_out)))
    if y is not None:
        if copy:
            from .stream import Trace

            tr = Trace(header=tr.stats.copy(), device_data=y)
        else:
            replace_samples(tr, y)
        tr.stats.sampling_rate = rate_out
        return tr
    out = tr.copy() if copy else tr
    out.data = resample_array(out.data, rate_in, rate_out)
    out.stats.sampling_rate = rate_out
    return out
