"""The spectrogram rule in float64, numpy only: the numeric content of the reference's ``spectrogram()``
(volpick/data/utils.py:1251-1440) up to the point where it starts to draw -- ``matplotlib.mlab.specgram`` of the demeaned
series plus the six lines behind it -- and the bound the device kernel (volpick_amd/csrc/spectrogram.hip) is held to.  Nothing
of the device code is used here.  tests/test_spectrogram_f64_cpu.py compares it with ``mlab.specgram`` itself and shows the
teeth of the bound.

The bound.  Let A_j be frame j's largest amplitude over all pad / 2 + 1 bins, bin 0 included, in the units of the amplitude
output.  A float64 FFT errs by about log2(pad) 2^-53 A_j per bin; 2^-40 A_j leaves some two orders of margin over that and is
still five orders under anything float32 arithmetic inside the kernel would produce.  The output is rounded once to float32
(2^-24 relative; 2^-23 allows for the reference value's own rounding).  So

    amplitude:  |got - want| <= 2^-23 |want| + 2^-40 A_j
    dB:         |got - want| <= 2^-23 |want| + (20 / ln 10) 2^-40 A_j / a        (a: the bin's amplitude; d(20 log10 a) = 20 / ln 10 da / a)

and -inf, 0 and NaN must match exactly.
"""
from __future__ import annotations

import math

import numpy as np


def nearest_pow_2(x):
    """The reference's ``_nearest_pow_2``: ties go down."""
    a = math.pow(2, math.ceil(np.log2(x)))
    b = math.pow(2, math.floor(np.log2(x)))
    return a if abs(a - x) < abs(b - x) else b


def plan(npts, samp_rate, per_lap=0.9, wlen=None, mult=8.0):
    """``(nfft, pad, nlap, hop, n_frames)``; ValueError where the reference raises, and where hop < 1 or hop > nfft."""
    samp_rate = float(samp_rate)
    if not wlen:
        wlen = 128 / samp_rate
    nfft = int(nearest_pow_2(wlen * samp_rate))
    if npts < nfft:
        raise ValueError(f"Input signal too short ({npts} samples, nfft {nfft} samples)")
    pad = nfft if mult is None else int(nearest_pow_2(mult)) * nfft
    nlap = int(nfft * float(per_lap))
    hop = nfft - nlap
    if hop < 1 or hop > nfft:
        raise ValueError(f"per_lap = {per_lap} leaves a hop of {hop} samples, need 1..{nfft}")
    n_frames = (npts - nlap) // hop
    if n_frames < 2:
        raise ValueError(f"Input signal too short ({npts} samples, nfft {nfft}, {nlap} samples overlap)")
    return nfft, pad, nlap, hop, n_frames


def axes(npts, samp_rate, nfft, pad, hop):
    freq = np.fft.fftfreq(pad, 1.0 / samp_rate)[1 : pad // 2 + 1].copy()
    freq[-1] = abs(freq[-1])
    time = np.arange(nfft / 2, npts - nfft / 2 + 1, hop) / samp_rate
    return freq, time


def _amplitudes(data, samp_rate, nfft, pad, hop, frames, dtype=np.float64, mean=None):
    """sqrt(P) of every bin 0 .. pad / 2 of frames [frames[0], frames[1]): (pad / 2 + 1, n).  ``dtype``: the precision of the
    windowing and the transform (float32: the arithmetic the bound must catch); ``mean``: subtracted instead of the series' own
    float64 mean (a float32 mean: likewise)."""
    x = np.asarray(data, dtype=np.float64)
    x = x - (x.mean() if mean is None else mean)
    w = np.hanning(nfft)
    fr = np.lib.stride_tricks.sliding_window_view(x, nfft)[::hop][frames[0] : frames[1]]
    if dtype == np.float32:
        import scipy.fft  # numpy < 2 transforms float32 input in float64; scipy keeps it single

        X = scipy.fft.fft((fr.astype(np.float32) * w.astype(np.float32)), n=pad, axis=1)[:, : pad // 2 + 1].astype(np.complex128)
    else:
        X = np.fft.fft(fr * w, n=pad, axis=1)[:, : pad // 2 + 1]
    P = (X.real**2 + X.imag**2) / samp_rate / (w**2).sum()
    P[:, 1 : pad // 2] *= 2.0
    return np.sqrt(P).T


def spectrogram_f64(data, samp_rate, per_lap=0.9, wlen=None, dbscale=False, mult=8.0, frames=None, _dtype=np.float64,
                    _mean=None):
    """``(specgram, freq, time, A)`` of one series: specgram (pad / 2, n_frames) float64, the axes, and A (n_frames,), each
    frame's largest amplitude over bins 0 .. pad / 2 (what `bound` takes).  ``frames = (start, stop)`` selects columns."""
    data = np.asarray(data)
    npts = len(data)
    samp_rate = float(samp_rate)
    nfft, pad, nlap, hop, n_frames = plan(npts, samp_rate, per_lap, wlen, mult)
    lo, hi = (0, n_frames) if frames is None else frames
    assert 0 <= lo <= hi <= n_frames
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        amp = _amplitudes(data, samp_rate, nfft, pad, hop, (lo, hi), _dtype, _mean)
        A = amp.max(axis=0) if amp.shape[1] else np.zeros(0)
        spec = 20.0 * np.log10(amp[1:]) if dbscale else amp[1:]  # 10 log10(P)
    freq, time = axes(npts, samp_rate, nfft, pad, hop)
    assert len(time) == n_frames
    return spec, freq, time[lo:hi], A


def bound(want, A, dbscale=False):
    """The largest |got - want| allowed per element; ``want`` (n_freq, n_frames) float64, ``A`` (n_frames,)."""
    want = np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if dbscale:
            a = 10.0 ** (want / 20.0)
            b = 2.0**-23 * np.abs(want) + (20.0 / math.log(10.0)) * 2.0**-40 * A[None, :] / a
        else:
            b = 2.0**-23 * np.abs(want) + 2.0**-40 * A[None, :]
    return b


def ratio(got, want, A, dbscale=False):
    """Worst |got - want| / bound over the elements; inf where -inf, 0 (a frame of zeros) or NaN do not match exactly."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return float("inf")
    exact = ~np.isfinite(want) | (A[None, :] == 0.0)
    if not np.array_equal(got[exact], want[exact], equal_nan=True):
        return float("inf")
    rest = ~exact
    if not rest.any():
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(got - want)[rest] / bound(want, A, dbscale)[rest]
    if np.isnan(r).any():
        return float("inf")
    return float(r.max())


def signal(n, seed, samp_rate=100.0, offset=50.0, amp=10.0):
    """Seeded noise of amplitude ``amp`` plus a 2 Hz and a 12 Hz burst, around ``offset``: float64 (n,)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * amp
    m = min(n // 4, int(6 * samp_rate))
    if m > 8:
        t = np.arange(m) / samp_rate
        env = np.exp(-t / 1.5) * 40.0 * amp
        for at, hz in ((n // 8, 2.0), (n // 2, 12.0)):
            x[at : at + m] += env * np.sin(2 * np.pi * hz * t)
    return x + offset
