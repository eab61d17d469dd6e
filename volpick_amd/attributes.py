"""Frequency index and signal-to-noise ratio of picks and bank traces, computed on the GPU.

The reference stores three attributes with every trace it writes (its volpick/data/convert.py:222-270, through
``freqency_index`` and ``calculate_snr`` of volpick/data/utils.py), and its evaluation bins the targets by them:

* ``trace_frequency_index`` -- log10 of the mean spectral amplitude in 10-15 Hz over that in 1-5 Hz, from 1 s before to 6 s
  after the onset (Hann window), averaged over the components that are neither dead nor NaN.  Long-period events sit well
  below volcano-tectonic ones.
* ``trace_snr_db`` / ``trace_mean_snr_db`` -- per component, 20 log10 of the 95th percentile of ``|x|`` in the 5 s behind the S
  onset (behind P where there is no usable S) over that in the 5 s ahead of P; and their ``nanmean``.

The work is split as in :mod:`volpick_amd.generate`.  :func:`plan_rows` decides on the host everything that follows from
lengths and onsets alone -- the three windows, the first bin and bin count of each band from ``fftfreq``'s own float64
values, the percentile's two indices and its weight -- and the kernel (``csrc/attributes.hip``, one workgroup per row,
float64, deterministic) does what depends on sample values.  :func:`bank_attributes` characterises every trace of a
:class:`~volpick_amd.generate.WaveformBank`, :func:`pick_attributes` every pick of a ``classify`` result, on the stream
the picks came from, device-resident or not.

Where the reference's own code would fail, a row is NaN instead: no reference sample (no onset, or the onsets that exist
are sample 0), an empty window, an empty band.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._device import stream_handle
from .stream import sample_offset

ATTR_ROW = np.dtype([
    ("trace", np.int32), ("flags", np.int32),
    ("fi_start", np.int64), ("noise_start", np.int64), ("signal_start", np.int64),
    ("fi_n", np.int32), ("noise_n", np.int32), ("signal_n", np.int32),
    ("lo_first", np.int32), ("lo_count", np.int32), ("hi_first", np.int32), ("hi_count", np.int32),
    ("noise_lo", np.int32), ("noise_up", np.int32), ("signal_lo", np.int32), ("signal_up", np.int32),
    ("reserved", np.int32), ("noise_g", np.float64), ("signal_g", np.float64)], align=True)
assert ATTR_ROW.itemsize == C.sizeof(_lib.VpAttrRow)

MAX_WINDOW = _lib.VP_ATTR_MAX_WINDOW
N_OUT = _lib.VP_ATTR_OUT
COLUMNS = ("trace_frequency_index", "trace_snr_db", "trace_mean_snr_db", "component_frequency_index")


def band_bins(n, sampling_rate, band):
    """(first, count) of the bins k < n // 2 with ``band[0] < fftfreq(n, 1 / sampling_rate)[k] < band[1]``, both strict, by
    the float64 values ``fftfreq`` itself returns (at n = 700, 100 Hz, bin 70 is exactly 10.0 and lies outside 10-15 Hz)."""
    if n < 2:
        return 0, 0
    freq = np.fft.fftfreq(n, 1.0 / sampling_rate)[: n // 2]
    k = np.flatnonzero((freq > band[0]) & (freq < band[1]))
    return (int(k[0]), len(k)) if len(k) else (0, 0)


def percentile_plan(m, q=95):
    """(lo, up, g): numpy's linear percentile of m sorted values is ``a[lo] + (a[up] - a[lo]) g`` (``a[up] - (a[up] - a[lo])
    (1 - g)`` where g >= 0.5)."""
    if m < 1:
        return 0, 0, 0.0
    h = (m - 1) * (q / 100)
    lo = math.floor(h)
    return lo, min(lo + 1, m - 1), h - lo


def plan_rows(lengths, p, s, sampling_rate, fi_window=(1.0, 6.0), low_band=(1, 5), high_band=(10, 15), snr_window=5.0,
              demean=False):
    """One :data:`ATTR_ROW` per trace of ``lengths`` samples with P onset ``p`` and S onset ``s`` (samples; NaN or None =
    missing); row i names trace i.

    Frequency index: the reference sample is P if it exists and is not 0, else S likewise, else none (NaN); the window is
    ``[max(ref - wb, 0), min(ref + wa, N))`` with ``wb, wa = fi_window`` seconds.  SNR: none if P is missing or below 10;
    noise ``[max(0, int(p - w)), p)`` with ``w = snr_window * sampling_rate``; signal ``[s, min(int(s + w), N))`` if S exists
    and ``s < N - 10``, else ``[p, min(int(p + w), N))``.  ``demean``: the kernel subtracts each component's mean over the
    span of the row's windows first (raw counts; bank traces are already demeaned)."""
    N = np.atleast_1d(np.asarray(lengths, np.int64))
    n_rows = len(N)
    sr = float(sampling_rate)
    wb, wa = int(round(fi_window[0] * sr)), int(round(fi_window[1] * sr))
    winlen = snr_window * sr

    def onsets(v):  # -> (present, the integer sample the reference stores: int(), toward zero)
        v = np.broadcast_to(np.asarray(np.nan if v is None else v, np.float64), (n_rows,))
        ok = np.isfinite(v)
        return ok, np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0.0)

    def trunc(v):
        return np.trunc(v).astype(np.int64)

    has_p, pf = onsets(p)
    has_s, sf = onsets(s)
    pi, si = pf.astype(np.int64), sf.astype(np.int64)
    if (has_s & (si < 0)).any():
        raise ValueError(f"row {int(np.flatnonzero(has_s & (si < 0))[0])}: an S onset at a negative sample")
    rows = np.zeros(n_rows, ATTR_ROW)
    rows["trace"] = np.arange(n_rows)
    rows["flags"] = _lib.VP_ATTR_DEMEAN if demean else 0
    # frequency index: the reference sample is P if truthy, else S if truthy
    use_p = has_p & (pi != 0)
    has_ref = use_p | (has_s & (si != 0))
    ref = np.where(use_p, pi, si)
    a, b = np.maximum(ref - wb, 0), np.minimum(ref + wa, N)
    n = np.where(has_ref & (b > a), b - a, 0)
    rows["fi_start"], rows["fi_n"] = np.where(n > 0, a, 0), n
    for v in np.unique(n[n > 0]):
        k = n == v
        (rows["lo_first"][k], rows["lo_count"][k]), (rows["hi_first"][k], rows["hi_count"][k]) = \
            band_bins(int(v), sr, low_band), band_bins(int(v), sr, high_band)
    # SNR: noise ahead of P; signal behind S where it is usable, else behind P
    valid = has_p & (pi >= 10)
    use_s = has_s & (si < N - 10)
    windows = {
        "noise": (np.minimum(np.maximum(0, trunc(pf - winlen)), N), np.minimum(pi, N)),
        "signal": (np.where(use_s, si, np.minimum(pi, N)), np.minimum(np.where(use_s, trunc(sf + winlen), trunc(pf + winlen)), N)),
    }
    for name, (a, b) in windows.items():
        m = np.where(valid, np.maximum(b - a, 0), 0)
        rows[name + "_start"], rows[name + "_n"] = np.where(m > 0, a, 0), m
        for v in np.unique(m[m > 0]):
            k = m == v
            rows[name + "_lo"][k], rows[name + "_up"][k], rows[name + "_g"][k] = percentile_plan(int(v))
    return rows


def as_rows(rows) -> np.ndarray:
    rows = np.asarray(rows)
    if rows.dtype != ATTR_ROW or rows.ndim != 1 or rows.size == 0:
        raise TypeError("attribute rows: a non-empty 1-D array of attributes.ATTR_ROW")
    return np.ascontiguousarray(rows)


def _columns(out):
    return {
        "trace_frequency_index": out[:, 3].copy(),
        "trace_snr_db": out[:, 10:13].copy(),
        "trace_mean_snr_db": out[:, 13].copy(),
        "component_frequency_index": out[:, 0:3].copy(),
    }


def array_attributes(data, rows, raw=False):
    """``vp_attributes`` on one (3, N) float32 CUDA tensor: the columns of :func:`bank_attributes` for ``rows``
    (``raw=True``: the kernel's (n_rows, 14) float64 table -- fi[3], fi_trace, noise_p95[3], signal_p95[3], snr_db[3],
    snr_mean)."""
    import torch

    if not (torch.is_tensor(data) and data.is_cuda and data.dtype == torch.float32 and data.dim() == 2 and data.shape[0] == 3):
        raise TypeError("array_attributes: a (3, N) float32 CUDA tensor")
    data = data.contiguous()
    rows = as_rows(rows)
    out = np.full((len(rows), N_OUT), np.nan)
    dev = data.device.index
    _lib.check(_lib.load().vp_attributes(dev, C.c_void_p(data.data_ptr()), data.shape[1], rows.ctypes.data_as(C.POINTER(_lib.VpAttrRow)),
                                         len(rows), out.ctypes.data_as(C.c_void_p), stream_handle(dev)), "vp_attributes")
    return out if raw else _columns(out)


def bank_attributes(bank, sampling_rate=100, fi_window=(1.0, 6.0), low_band=(1, 5), high_band=(10, 15), snr_window=5.0,
                    raw=False):
    """The reference's attribute columns for every trace of a :class:`~volpick_amd.generate.WaveformBank`, from its first
    P and first S onset (truncated with ``int()`` as the reference stores them): ``trace_frequency_index`` (N,),
    ``trace_snr_db`` (N, 3), ``trace_mean_snr_db`` (N,) and ``component_frequency_index`` (N, 3), float64 on the host."""
    rows = plan_rows(bank.lengths, bank.onsets[:, 0], bank.onsets[:, 2], sampling_rate, fi_window, low_band, high_band,
                     snr_window, demean=False)
    out = np.full((len(rows), N_OUT), np.nan)
    _lib.check(_lib.load().vp_bank_attributes(bank.handle, rows.ctypes.data_as(C.POINTER(_lib.VpAttrRow)), len(rows),
                                              out.ctypes.data_as(C.c_void_p), stream_handle(bank.device)),
               "vp_bank_attributes")
    return out if raw else _columns(out)


def pick_attributes(stream, picks, sampling_rate=100, component_order="ZNE", in_samples=3001, fi_window=(1.0, 6.0),
                    low_band=(1, 5), high_band=(10, 15), snr_window=5.0, device=0, raw=False):
    """The same columns for every pick of ``picks`` (a ``PickList``, or anything whose items have ``trace_id`` and
    ``peak_time``), aligned with ``picks``, read from ``stream`` -- host traces or device-backed ones, which stay on the
    device.  The blocks are formed as the picker forms them (``_group_stream`` at ``sampling_rate`` on a copy); a pick lies
    in the block of its ``trace_id`` at sample ``round((peak_time - block start) * sampling_rate)``.  Each pick is
    characterised on its own: its sample is the reference sample and the P onset, there is no S, and the windows are
    demeaned (raw counts carry an offset).  A pick that falls in no block is a NaN row.  One launch per block."""
    import torch

    from .models import _group_stream

    picks = list(picks)
    out = np.full((len(picks), N_OUT), np.nan)
    done = np.zeros(len(picks), bool)
    by_id = {}
    for i, pk in enumerate(picks):
        if getattr(pk, "peak_time", None) is not None:
            by_id.setdefault(pk.trace_id, []).append(i)
    for grp in _group_stream(stream, component_order, sampling_rate, True, in_samples):
        n = int(grp["data"].shape[1])
        idx, samples = [], []
        for i in by_id.get(grp["trace_id"], ()):
            k = sample_offset(picks[i].peak_time, grp["starttime"], sampling_rate)
            if 0 <= k < n and not done[i]:
                idx.append(i)
                samples.append(k)
        if not idx:
            continue
        data = grp["data"]
        if not torch.is_tensor(data):
            data = torch.from_numpy(np.ascontiguousarray(np.asarray(data, np.float32))).to(torch.device("cuda", device))
        rows = plan_rows(np.full(len(idx), n), samples, None, sampling_rate, fi_window, low_band, high_band, snr_window,
                         demean=True)
        rows["trace"] = 0
        out[idx] = array_attributes(data, rows, raw=True)
        done[idx] = True
    return out if raw else _columns(out)
