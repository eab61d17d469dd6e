"""The float64 answer, the bounds and an emulation of the kernel's order that the CPU and GPU tests of the attribute kernel
share (volpick_amd/csrc/attributes.hip, ``vp_attributes`` / ``vp_bank_attributes``).  Numpy and scipy only; nothing here
touches the device code or ``volpick_amd.attributes``' planner (the tests compare the two).

The rule (the reference's ``freqency_index`` / ``calculate_snr`` and their call site, restated):

Frequency index of one component ``x`` (length N, rate sr) at the reference sample ``ref``: the window is
``x[max(ref - wb, 0) : min(ref + wa, N)]`` (n samples, wb = 1 sr, wa = 6 sr); ``spec = fft(window * hann(n))[:n // 2]`` with
scipy's symmetric Hann; ``freq = fftfreq(n, 1 / sr)[:n // 2]``; ``A_up = mean |spec|`` over ``10 < freq < 15``, ``A_low`` over
``1 < freq < 5``, all four comparisons strict; ``FI = log10(A_up / A_low)``.  A component whose ``sum |diff(x)|`` over the whole
component is ``<= 1e-9`` is skipped (a NaN sum is not: a NaN outside the window leaves the component in, where the reference's
``> 1e-9`` would drop it), and so is one whose FI is NaN; the trace's FI is the mean of the rest, NaN if none.
``ref`` is the P sample if truthy, else the S sample if truthy, else the row is NaN.  An empty band or window gives NaN.

SNR with ``winlen = 5 sr``: P missing or below 10 -> everything NaN.  Noise ``|x[max(0, int(p - winlen)) : p]|``; signal
``|x[s : min(int(s + winlen), N)]|`` if S exists and ``s < N - 10``, else ``|x[p : min(int(p + winlen), N)]|``; ``noi``, ``sig``
their 95th percentiles (numpy's default linear method); a component is NaN where ``np.isclose(noi, 0)`` or
``np.isclose(sig, 0)``, else ``20 log10(sig / noi)``; the mean is ``nanmean``, NaN when all three are.

``demean`` (the stream surface): per component, the float64 mean over the span from the earliest window start to the latest
window end is subtracted before both computations.

Bounds, none of them taken from a run of the kernel:

* FI, per component: a float64 sum of n products errs by at most about ``n 2^-53 sum |terms|``; with ``S = sum |x_j w_j|`` every
  ``|X[k]|`` is good to ``(n + 8) 2^-52 S`` (twice the worst case; the 8 covers the unit roots' last bit), so
  ``|dFI| <= (2 / ln 10) (n + 8) 2^-52 S / min(A_up, A_low)``.  The trace's FI is a mean of components: the largest of theirs.
* percentiles without demean: equal to numpy's bit for bit.
* SNR: ``|d snr_db| <= 2^-46 max(1, |snr_db|)`` (division and log10 give about 2^-50 absolute at 20 dB per decade; the factor
  16 covers the device log10's last bits).
* with demean: the device's mean may differ from numpy's pairwise mean by ``e = L 2^-53 max|x|`` (L the span).  The percentiles
  may move by ``2 e``; S grows by ``e sum w``; and since d(20 log10(sig / noi)) = (20 / ln 10)(d sig / sig - d noi / noi), the
  SNR bound grows by ``(20 / ln 10) 2 e (1 / sig + 1 / noi)``.
"""
import math
import warnings

import numpy as np
import scipy.fft
from scipy.signal import windows

OUT_FI, OUT_FI_TRACE, OUT_NOISE, OUT_SIGNAL, OUT_SNR, OUT_SNR_MEAN = slice(0, 3), 3, slice(4, 7), slice(7, 10), slice(10, 13), 13
N_OUT = 14
EPS52, EPS53, EPS46 = 2.0 ** -52, 2.0 ** -53, 2.0 ** -46
LOW_BAND, HIGH_BAND = (1, 5), (10, 15)


def _missing(v):
    return v is None or (isinstance(v, float) and math.isnan(v)) or (isinstance(v, np.floating) and np.isnan(v))


def _int(v):
    return None if _missing(v) else int(v)


def frequency_index(data, dt, low_band=LOW_BAND, high_band=HIGH_BAND, detail=False):
    """FI of one window (float64).  detail: also (S, A_up, A_low)."""
    data = np.asarray(data, np.float64)
    n = len(data)
    if n == 0:
        return (np.nan, 0.0, np.nan, np.nan) if detail else np.nan
    win = windows.hann(n)
    xw = data * win
    spec = scipy.fft.fft(xw)[0 : n // 2]
    freq = scipy.fft.fftfreq(n, dt)[0 : n // 2]
    amp = np.abs(spec)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        a_up = np.mean(amp[np.logical_and(freq > high_band[0], freq < high_band[1])])
        a_low = np.mean(amp[np.logical_and(freq > low_band[0], freq < low_band[1])])
        fi = np.log10(a_up / a_low)
    return (fi, float(np.abs(xw).sum()), a_up, a_low) if detail else fi


def windows_of(n_samples, p, s, sr=100, fi_window=(1.0, 6.0), snr_window=5.0):
    """{"fi", "noise", "signal"}: (start, stop) or None, by the rule above."""
    N, p, s = int(n_samples), _int(p), _int(s)
    out = {"fi": None, "noise": None, "signal": None}
    ref = p if p else (s if s else None)
    if ref is not None:
        a, b = max(ref - int(round(fi_window[0] * sr)), 0), min(ref + int(round(fi_window[1] * sr)), N)
        if b > a:
            out["fi"] = (a, b)
    winlen = snr_window * sr
    if p is not None and p >= 10:
        out["noise"] = (min(max(0, int(p - winlen)), N), min(int(p), N))
        if s is not None and s < N - 10:
            out["signal"] = (int(s), min(int(s + winlen), N))
        else:
            out["signal"] = (min(int(p), N), min(int(p + winlen), N))
    return out


def _p95(a):
    if len(a) == 0:
        return np.nan
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return float(np.percentile(a, 95))


def trace_attributes(x, p, s, sr=100, fi_window=(1.0, 6.0), low_band=LOW_BAND, high_band=HIGH_BAND, snr_window=5.0,
                     demean=False):
    """x: (3, N).  -> (out, tol): out the 14 values in the kernel's order (fi[3], fi_trace, noise_p95[3], signal_p95[3],
    snr_db[3], snr_mean), tol the bound on each of them (0 = bit for bit)."""
    x = np.asarray(x, np.float64)
    N = x.shape[1]
    w = windows_of(N, p, s, sr, fi_window, snr_window)
    out, tol = np.full(N_OUT, np.nan), np.zeros(N_OUT)
    with np.errstate(all="ignore"):
        flat = [bool(np.sum(np.abs(np.diff(c))) <= 1e-9) for c in x]  # over the WHOLE component; a NaN sum does not skip
    e = 0.0
    if demean:
        spans = [v for v in w.values() if v is not None and v[1] > v[0]]
        if spans:
            lo, hi = min(v[0] for v in spans), max(v[1] for v in spans)
            with np.errstate(all="ignore"):
                e = (hi - lo) * EPS53 * float(np.nanmax(np.abs(x[:, lo:hi])))
                x = x - x[:, lo:hi].mean(axis=1, keepdims=True)
    # frequency index
    fis, tols = [], []
    if w["fi"] is not None:
        a, b = w["fi"]
        n = b - a
        for c in range(3):
            fi, S, a_up, a_low = frequency_index(x[c, a:b], 1.0 / sr, low_band, high_band, detail=True)
            if flat[c] or np.isnan(fi):
                continue
            out[c] = fi
            S += e * float(windows.hann(n).sum())
            tol[c] = (2.0 / math.log(10.0)) * (n + 8) * EPS52 * S / min(a_up, a_low)
            fis.append(fi)
            tols.append(tol[c])
    if fis:
        out[OUT_FI_TRACE] = np.mean(fis)
        tol[OUT_FI_TRACE] = max(tols)
    # percentiles and SNR
    if w["noise"] is not None:
        snrs = []
        for c in range(3):
            noi = _p95(np.abs(x[c, w["noise"][0] : w["noise"][1]]))
            sig = _p95(np.abs(x[c, w["signal"][0] : w["signal"][1]]))
            out[4 + c], out[7 + c] = noi, sig
            tol[4 + c] = tol[7 + c] = 2 * e
            with np.errstate(all="ignore"):
                if np.isclose(noi, 0) or np.isclose(sig, 0):
                    snrs.append(np.nan)
                else:
                    snrs.append(20 * np.log10(sig / noi))
                    if np.isfinite(snrs[-1]):
                        tol[10 + c] = EPS46 * max(1.0, abs(snrs[-1])) + (20.0 / math.log(10.0)) * 2 * e * (1 / sig + 1 / noi)
        out[OUT_SNR] = snrs
        if not np.all(np.isnan(snrs)):
            out[OUT_SNR_MEAN] = np.nanmean(snrs)
            tol[OUT_SNR_MEAN] = np.nanmax(tol[OUT_SNR])
    return out, tol


def ratio(got, want, tol):
    """Worst |got - want| / tol over the 14 values (0 where both are equal, inf where the NaN pattern or an exact value
    differs)."""
    got, want, tol = (np.asarray(v, np.float64).ravel() for v in (got, want, tol))
    if got.shape != want.shape or (np.isnan(got) != np.isnan(want)).any():
        return float("inf")
    ok = ~np.isnan(want)
    with np.errstate(all="ignore"):
        d = np.abs(got[ok] - want[ok])
        d[got[ok] == want[ok]] = 0.0  # equal infinities
    t = tol[ok]
    r = np.where(d == 0, 0.0, np.where(t > 0, d / np.where(t > 0, t, 1.0), np.inf))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's order, in numpy: direct DFT at the planned bins with a table of n unit roots and the phase walked in
# integers, sequential sums, magnitudes, band means in bin order; percentiles by rank counting.
def unit_roots(n, dtype=np.float64):
    r = np.arange(n, dtype=np.float64)
    return (np.cos(np.pi * (2 * r / n)) - 1j * np.sin(np.pi * (2 * r / n))).astype(np.complex128 if dtype == np.float64 else np.complex64)


def hann_kernel(n):
    """The window as the kernel forms it: sin^2(pi j / (n - 1)), [1.0] for n = 1."""
    return np.ones(1) if n == 1 else np.sin(np.pi * (np.arange(n) / (n - 1))) ** 2


def emulate_fi(data, lo_first, lo_count, hi_first, hi_count, dtype=np.float64):
    """FI of one window in the kernel's order, every product and sum in `dtype`."""
    n = len(data)
    xw = (np.asarray(data, np.float64) * hann_kernel(n)).astype(dtype)
    roots = unit_roots(n, dtype)
    k = np.concatenate([np.arange(lo_first, lo_first + lo_count), np.arange(hi_first, hi_first + hi_count)])
    re, im, r = np.zeros(len(k), dtype), np.zeros(len(k), dtype), np.zeros(len(k), np.int64)
    for j in range(n):
        wr = roots[r]
        re = re + xw[j] * wr.real.astype(dtype)
        im = im + xw[j] * wr.imag.astype(dtype)
        r = (r + k) % n
    mag = np.hypot(re, im).astype(dtype)
    a_low, a_up = dtype(0), dtype(0)
    for v in mag[:lo_count]:
        a_low = a_low + v
    for v in mag[lo_count:]:
        a_up = a_up + v
    with np.errstate(all="ignore"):
        return float(np.log10((a_up / dtype(hi_count)) / (a_low / dtype(lo_count))))


def longdouble_fi(data, lo_first, lo_count, hi_first, hi_count):
    """(FI, S, A_up, A_low) of one window by a direct DFT in extended precision, scipy's window."""
    n = len(data)
    ld = np.longdouble
    xw = np.asarray(data, np.float64).astype(ld) * windows.hann(n).astype(ld)
    pi = 4 * np.arctan(ld(1))
    j = np.arange(n, dtype=np.int64)
    amps = []
    for k in list(range(lo_first, lo_first + lo_count)) + list(range(hi_first, hi_first + hi_count)):
        ph = 2 * pi * ((j * k) % n).astype(ld) / ld(n)
        amps.append(np.hypot((xw * np.cos(ph)).sum(), (xw * np.sin(ph)).sum()))
    amps = np.array(amps, ld)
    a_low, a_up = amps[:lo_count].mean(), amps[lo_count:].mean()
    return float(np.log10(a_up / a_low)), float(np.abs(xw).sum()), float(a_up), float(a_low)


def fi_bound(n, S, a_up, a_low):
    return (2.0 / math.log(10.0)) * (n + 8) * EPS52 * S / min(a_up, a_low)


def emulate_percentile(a, lo, up, g):
    """The planned percentile by rank counting (ties broken by index) and numpy's interpolation order."""
    a = np.asarray(a, np.float64)
    if np.isnan(a).any():
        return np.nan
    idx = np.arange(len(a))
    rank = (a[None, :] < a[:, None]).sum(1) + ((a[None, :] == a[:, None]) & (idx[None, :] < idx[:, None])).sum(1)
    va, vb = a[rank == lo][0], a[rank == up][0]
    d = vb - va
    return vb - d * (1 - g) if g >= 0.5 else va + d * g


def noise(n, seed, decades=0.0, offset=0.0):
    """(3, n) float32: white noise scaled by 10^decades plus an offset, a little low-passed so that the bands differ."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, n + 2))
    x = (x[:, 2:] + 0.6 * x[:, 1:-1] + 0.3 * x[:, :-2]) * 10.0 ** decades + offset
    return x.astype(np.float32)
