"""Spectrograms of device-resident traces -- the numbers of the reference's ``spectrogram()`` (volpick/data/utils.py:1251-1440;
ObsPy's ``obspy.imaging.spectrogram``) up to the point where that function starts to draw: ``matplotlib.mlab.specgram`` of the
demeaned series with a Hann window of ``nfft`` samples zero-padded to ``pad``, bin 0 dropped, then ``sqrt`` or ``10 log10``.
Everything behind ``specgram = ...`` in the reference (``clip``, ``Normalize``, axes, colormaps, files, ``log``) is drawing and
out of scope.

:func:`plan` is pure host code: ``nfft``, ``pad``, ``nlap``, ``hop`` and the frame count from the length and the rate alone.
:func:`spectrogram` runs ``vp_spectrogram`` (volpick_amd/csrc/spectrogram.hip: float64 throughout, one rounding to float32 at
the store) on one series or a batch of equal-length series and returns a :class:`Spectrogram` ``(data, freq, time)``;
``data[..., f, t]`` is frequency-major as the reference's ``specgram[f, t]``, without the ``flipud`` of its drawing branch.
There is no host fallback: a host trace is uploaded and goes through the same kernel.

The one deviation from the reference: for float32 input its ``data.mean()`` accumulates in float32; the mean here is a float64
sum in a fixed order, whatever the input's dtype.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np

from . import _lib
from ._device import SAMPLE_KINDS, device_backing, release_scratch, stream_handle, upload_samples

TILE_FRAMES = _lib.VP_SPECTROGRAM_TILE_FRAMES  # consecutive frames a workgroup of the kernel owns (at nfft <= 128)


class Spectrogram(NamedTuple):
    data: object      # float32 CUDA tensor (..., n_freq, n_frames)
    freq: np.ndarray  # float64 (n_freq,): fftfreq's bins 1 .. pad / 2, the last one positive
    time: np.ndarray  # float64 (n_frames,): frame centres in seconds from the first sample


def tile_frames(nfft):
    """Frames per workgroup of the kernel at window length ``nfft``."""
    return min(TILE_FRAMES, 4096 // int(nfft))


def _nearest_pow_2(x):
    """The reference's ``_nearest_pow_2``: the power of two nearest to ``x``, ties go down."""
    a = math.pow(2, math.ceil(np.log2(x)))
    b = math.pow(2, math.floor(np.log2(x)))
    return a if abs(a - x) < abs(b - x) else b


def plan(npts, samp_rate, per_lap=0.9, wlen=None, mult=8.0):
    """``(nfft, pad, nlap, hop, n_frames)`` as the reference forms them.  ``ValueError`` where the reference raises (fewer
    samples than one window, fewer than two frames) and where ``per_lap`` leaves no hop of 1..nfft samples."""
    samp_rate = float(samp_rate)
    if not (math.isfinite(samp_rate) and samp_rate > 0):
        raise ValueError(f"samp_rate = {samp_rate} is not finite and positive")
    if not wlen:
        wlen = 128 / samp_rate
    nfft = int(_nearest_pow_2(wlen * samp_rate))
    npts = int(npts)
    if npts < nfft:
        raise ValueError(f"Input signal too short ({npts} samples, window length {wlen} seconds, nfft {nfft} samples, "
                         f"sampling rate {samp_rate} Hz)")
    pad = nfft if mult is None else int(_nearest_pow_2(mult)) * nfft
    nlap = int(nfft * float(per_lap))
    hop = nfft - nlap
    if hop < 1 or hop > nfft:
        raise ValueError(f"per_lap = {per_lap} leaves a hop of {hop} samples; need 1..{nfft}")
    n_frames = (npts - nlap) // hop
    if n_frames < 2:
        raise ValueError(f"Input signal too short ({npts} samples, window length {wlen} seconds, nfft {nfft} samples, {nlap} "
                         f"samples window overlap, sampling rate {samp_rate} Hz)")
    return nfft, pad, nlap, hop, n_frames


def axes(npts, samp_rate, nfft, pad, hop):
    """``(freq, time)`` of the full result, float64, as ``mlab.specgram`` returns them (``freq`` without bin 0)."""
    freq = np.fft.fftfreq(pad, 1.0 / float(samp_rate))[1 : pad // 2 + 1].copy()
    freq[-1] = abs(freq[-1])  # fftfreq gives the Nyquist bin a minus sign
    time = np.arange(nfft / 2, npts - nfft / 2 + 1, hop) / float(samp_rate)
    return freq, time


def _series_layout(x):
    """``(n_series, series_stride, lead shape)`` of a CUDA tensor (..., N) that the library can read where it lies."""
    import torch

    if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 1 and str(x.dtype) in SAMPLE_KINDS):
        raise TypeError("spectrogram: need a Trace or a CUDA tensor (..., N) of int32, float32 or float64 samples")
    n = int(x.shape[-1])
    if n > 1 and x.stride(-1) != 1:
        raise ValueError("spectrogram: the tensor is not contiguous in its last dimension")
    lead = [(int(s), int(t)) for s, t in zip(x.shape[:-1], x.stride()[:-1]) if s != 1]
    if any(s == 0 for s, _ in lead):
        raise ValueError("spectrogram: the tensor holds no series")
    for (_, t0), (s1, t1) in zip(lead, lead[1:]):
        if t0 != s1 * t1:
            raise ValueError("spectrogram: the series do not lie at equal strides (make the tensor contiguous)")
    stride = lead[-1][1] if lead else n
    if lead and stride < n:
        raise ValueError("spectrogram: the series overlap")
    return int(np.prod([s for s, _ in lead], dtype=np.int64)) if lead else 1, stride, tuple(int(s) for s in x.shape[:-1])


def spectrogram(x, samp_rate=None, per_lap=0.9, wlen=None, dbscale=False, mult=8.0, frames=None):
    """The reference's ``spectrogram(data, samp_rate, per_lap, wlen, dbscale=dbscale, mult=mult)`` as numbers, on the GPU.

    ``x``: a ``volpick_amd.Trace`` (the rate comes from its stats; see :meth:`Trace.spectrogram`) or a CUDA tensor ``(..., N)``
    of int32, float32 or float64 samples, contiguous in its last dimension and with its series at equal strides -- a ``(3, N)``
    block or an ``(M, 3, L)`` bank tensor is one launch.  ``frames = (start, stop)`` computes those columns only: they equal
    ``full.data[..., start:stop]`` bit for bit (the mean is still the whole series'), so a day can be produced in pieces.

    Returns :class:`Spectrogram`: ``data`` float32 on the tensor's device ``(..., pad / 2, n_frames)``, written on torch's
    current stream (the call returns after the work is done); ``freq`` and ``time`` float64 on the host.  A NaN or Inf anywhere
    in a series makes that series' whole output NaN; a frame of exact zeros gives 0, or ``-inf`` with ``dbscale``.
    ``ValueError`` as the reference (too short), ``VolpickHipError`` where the library refuses (``nfft`` outside 32..512,
    ``pad / nfft`` above 16, ``pad`` above 4096)."""
    import torch

    from .stream import Trace

    if isinstance(x, Trace):
        return trace_spectrogram(x, per_lap=per_lap, wlen=wlen, dbscale=dbscale, mult=mult, frames=frames)
    if samp_rate is None:
        raise TypeError("spectrogram: samp_rate is required for a tensor")
    n_series, stride, lead = _series_layout(x)
    npts = int(x.shape[-1])
    samp_rate = float(samp_rate)
    nfft, pad, _, hop, n_frames = plan(npts, samp_rate, per_lap, wlen, mult)
    lo, hi = (0, n_frames) if frames is None else (int(frames[0]), int(frames[1]))
    if not 0 <= lo <= hi <= n_frames:
        raise ValueError(f"spectrogram: frames = ({lo}, {hi}) outside the {n_frames} frames of the series")
    freq, time = axes(npts, samp_rate, nfft, pad, hop)
    with torch.cuda.device(x.device):
        out = torch.empty(lead + (pad // 2, hi - lo), dtype=torch.float32, device=x.device)
        if hi > lo:  # an empty tensor has no address to hand over
            _lib.check(_lib.load().vp_spectrogram(
                x.device.index, C.c_void_p(x.data_ptr()), SAMPLE_KINDS[str(x.dtype)], n_series, stride, npts, samp_rate, nfft,
                pad, hop, int(bool(dbscale)), lo, hi - lo, C.c_void_p(out.data_ptr()), stream_handle(x.device)), "vp_spectrogram")
    return Spectrogram(out, freq, time[lo:hi])


def trace_spectrogram(tr, device=0, **kw):
    """:func:`spectrogram` of a ``Trace``.  A device-backed trace is read where it lies (no host copy is materialised); a host
    trace is uploaded to ``cuda:device`` in its own dtype (int32, float32, float64; anything else as float32) and goes through
    the same kernel.  Masked traces are refused (split the stream at its gaps first)."""
    import torch

    kw.pop("samp_rate", None)
    dev = device_backing(tr)
    if dev is None:
        dev = upload_samples(tr.data, torch.device("cuda", int(device)), "masked traces have no spectrogram")
    elif str(dev.dtype) not in SAMPLE_KINDS:
        dev = dev.to(torch.float32)
    return spectrogram(dev, float(tr.stats.sampling_rate), **kw)


def release_spectrogram_scratch(device=0):
    """Free the scratch :func:`spectrogram` keeps per device between calls; returns the bytes freed."""
    return release_scratch("vp_spectrogram_release_scratch", device)
