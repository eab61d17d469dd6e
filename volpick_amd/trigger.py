"""STA/LTA characteristic functions and the triggers cut from them, named as ``obspy.signal.trigger`` names them: what the
reference's waveform check (``volpick/data/utils.py:1064-1071``) applies to every component,

    cft = recursive_sta_lta(tr.data, min(int(5 * sr), n), min(int(20 * sr), n));  trigger_onset(cft, 2, 0.5)

A numpy array takes the host restatement (float64 numpy / scipy, what ObsPy computes); a CUDA tensor goes to the library
(``vp_sta_lta`` / ``vp_trigger_onset``, volpick_amd/csrc/stalta.hip: float64 arithmetic on the device) and the result stays on
the device.  :func:`trace_trigger` is ``Trace.trigger``; :func:`sta_lta_triggers` is the reference's check in one call.  There
is no silent host fallback inside the device functions: where the library refuses they raise ``VolpickHipError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._device import (SAMPLE_KINDS, device_samples, is_cuda, release_scratch, sample_args, trace_in_place, trace_samples,
                      try_on_device)

TINY = float(np.finfo(np.float64).tiny)
TYPES = {"classicstalta": _lib.VP_STALTA_CLASSIC, "recstalta": _lib.VP_STALTA_RECURSIVE}
_I64 = C.POINTER(C.c_int64)


def _check_windows(nsta, nlta):
    nsta, nlta = int(nsta), int(nlta)
    if not 1 <= nsta <= nlta:
        raise ValueError(f"need 1 <= nsta <= nlta, got nsta = {nsta}, nlta = {nlta}")
    return nsta, nlta


def _host_samples(a):
    a = np.asanyarray(a)
    if a.ndim != 1:
        raise ValueError("the host path takes one 1-D series")
    if isinstance(a, np.ma.MaskedArray) and np.ma.is_masked(a):
        raise NotImplementedError("masked samples: split the stream at its gaps first")
    return np.asarray(a, dtype=np.float64)


def _classic_host(a, nsta, nlta):
    """``classic_sta_lta_py``: windows as differences of the whole-trace cumulative sum, float64."""
    n = len(a)
    sta = np.cumsum(a * a)
    lta = sta.copy()
    sta[nsta:] = sta[nsta:] - sta[:-nsta]
    sta /= nsta
    lta[nlta:] = lta[nlta:] - lta[:-nlta]
    lta /= nlta
    sta[:min(nlta - 1, n)] = 0.0
    lta[lta < TINY] = TINY
    return sta / lta


def _recursive_host(a, nsta, nlta):
    """``recursive_sta_lta_py`` with both recursions as ``scipy.signal.lfilter``; ``lta``'s start value rides ``zi``.  0 where
    ``sta`` is 0: the rule's 0 / lta, also behind the sample where ``tiny (1 - clta)^i`` has left the doubles."""
    from scipy.signal import lfilter

    n = len(a)
    cft = np.zeros(n)
    if n < 2:
        return cft
    sq = a[1:] * a[1:]  # sample 0 never enters the sums
    csta, clta = 1.0 / nsta, 1.0 / nlta
    sta, _ = lfilter([csta], [1.0, -(1.0 - csta)], sq, zi=[0.0])
    lta, _ = lfilter([clta], [1.0, -(1.0 - clta)], sq, zi=[(1.0 - clta) * TINY])
    with np.errstate(invalid="ignore", divide="ignore"):
        np.divide(sta, lta, out=cft[1:], where=sta != 0.0)
    cft[:min(nlta, n)] = 0.0
    return cft


def sta_lta_device(x, type, nsta, nlta, dtype=None):
    """``vp_sta_lta`` on a CUDA tensor ``(n,)`` or ``(n_series, n)`` of int32, float32 or float64 samples (rows ``n`` or more
    apart); returns a new CUDA tensor of the same shape, float64 unless ``dtype=torch.float32``."""
    import torch

    if type not in TYPES:
        raise ValueError(f"trigger type {type!r} is not one of {sorted(TYPES)}")
    nsta, nlta = _check_windows(nsta, nlta)
    x = device_samples(x, "sta_lta_device", dims=(1, 2))
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("sta_lta_device: dtype is torch.float32 or torch.float64")
    n_series = int(x.shape[0]) if x.dim() == 2 else 1
    out = torch.empty_like(x, dtype=dtype)
    if out.numel() == 0:
        return out
    device, ptr, kind, n = sample_args(x)
    _lib.check(_lib.load().vp_sta_lta(device, ptr, kind, n_series, n, n, TYPES[type], nsta, nlta, C.c_void_p(out.data_ptr()),
                                      SAMPLE_KINDS[str(dtype)]), "vp_sta_lta")
    return out


def classic_sta_lta(a, nsta, nlta, dtype=None):
    """ObsPy's ``classic_sta_lta``.  numpy in, float64 numpy out (host); CUDA tensor in, CUDA tensor out (``vp_sta_lta``)."""
    if is_cuda(a):
        return sta_lta_device(a, "classicstalta", nsta, nlta, dtype)
    nsta, nlta = _check_windows(nsta, nlta)
    return _classic_host(_host_samples(a), nsta, nlta)


def recursive_sta_lta(a, nsta, nlta, dtype=None):
    """ObsPy's ``recursive_sta_lta``.  numpy in, float64 numpy out (host); CUDA tensor in, CUDA tensor out (``vp_sta_lta``)."""
    if is_cuda(a):
        return sta_lta_device(a, "recstalta", nsta, nlta, dtype)
    nsta, nlta = _check_windows(nsta, nlta)
    return _recursive_host(_host_samples(a), nsta, nlta)


def _pick_host(x, thr1, thr2):
    """(on, off, peak, value) of the host mirror ``vp_pick_host`` on a float32 array."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lib = _lib.load()
    cap = max(1, len(x) // 2 + 1)  # a trigger needs a sample above and one below before the next
    on, off, pk = (np.zeros(cap, np.int64) for _ in range(3))
    val = np.zeros(cap, np.float32)
    n = C.c_int(0)
    _lib.check(lib.vp_pick_host(x.ctypes.data_as(C.c_void_p), len(x), thr1, thr2, on.ctypes.data_as(_I64), off.ctypes.data_as(_I64),
                                pk.ctypes.data_as(_I64), val.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)), "vp_pick_host")
    k = min(n.value, cap)
    return on[:k], off[:k], pk[:k], val[:k]


def trigger_onset_device(cft, thr_on, thr_off, cap_per_series=1024):
    """``vp_trigger_onset`` on a float32 CUDA tensor ``(n,)`` or ``(n_series, n)``: ``(on, off, peak, value, series_of)`` as
    numpy arrays, grouped by series and sorted by onset.  Calls again with more room where a series holds more triggers
    than ``cap_per_series``."""
    import torch

    if not (torch.is_tensor(cft) and cft.is_cuda and cft.dim() in (1, 2) and cft.dtype == torch.float32):
        raise TypeError("trigger_onset on the device takes a 1-D or 2-D float32 CUDA tensor")
    if thr_off > thr_on:
        raise ValueError("thr2 > thr1 is the general rule of the host path: trigger_onset(cft.cpu().numpy(), thr1, thr2)")
    cft = cft.contiguous()
    n = int(cft.shape[-1])
    n_series = int(cft.shape[0]) if cft.dim() == 2 else 1
    if n_series == 0 or n == 0:
        return (np.zeros(0, np.int64),) * 3 + (np.zeros(0, np.float32), np.zeros(0, np.int32))
    torch.cuda.current_stream(cft.device).synchronize()
    lib = _lib.load()
    per = max(1, int(cap_per_series))
    while True:
        cap = per * n_series
        on, off, pk = (np.zeros(cap, np.int64) for _ in range(3))
        val, ser, found = np.zeros(cap, np.float32), np.zeros(cap, np.int32), C.c_int(0)
        _lib.check(lib.vp_trigger_onset(
            cft.device.index, C.c_void_p(cft.data_ptr()), n_series, n, n, thr_on, thr_off, on.ctypes.data_as(_I64),
            off.ctypes.data_as(_I64), pk.ctypes.data_as(_I64), val.ctypes.data_as(C.POINTER(C.c_float)),
            ser.ctypes.data_as(C.POINTER(C.c_int32)), per, cap, C.byref(found)), "vp_trigger_onset")
        if found.value <= cap:
            k = found.value
            return on[:k], off[:k], pk[:k], val[:k], ser[:k]
        per = max(2 * per, found.value)  # no series holds more than were found in all


def trigger_onset(cft, thr1, thr2, max_len=None, **kw):
    """ObsPy's ``trigger_onset``: an ``(m, 2)`` int64 array of on / off samples (empty: shape ``(0, 2)``).  A numpy array goes
    to the host mirror (``vp_pick_host``, the general rule); a 1-D float32 CUDA tensor goes to ``vp_trigger_onset``, which has
    the rule for ``thr2 <= thr1`` without ``max_len``."""
    if is_cuda(cft):
        if max_len is not None or kw:
            raise ValueError("max_len is not available on the device: use the host path, trigger_onset(cft.cpu().numpy(), ...), "
                             "and cut the triggers there")
        if cft.dim() != 1:
            raise ValueError("trigger_onset takes one series; trigger_onset_device takes several")
        on, off = trigger_onset_device(cft, float(thr1), float(thr2))[:2]
    else:
        if max_len is not None or kw:
            raise NotImplementedError("max_len: cut the triggers of trigger_onset(cft, thr1, thr2) to length instead")
        cft = np.asarray(cft)
        if cft.ndim != 1:
            raise ValueError("trigger_onset takes one series")
        on, off = _pick_host(cft, float(thr1), float(thr2))[:2]
    return np.stack([on, off], axis=1).astype(np.int64).reshape(-1, 2)


def _windows(tr, sta, lta):
    """``nsta``, ``nlta`` in samples, clipped to ``[1, npts]`` as the reference clips them."""
    sr, n = float(tr.stats.sampling_rate), max(int(tr.stats.npts), 1)
    clip = lambda v: min(max(int(v * sr), 1), n)  # noqa: E731
    return clip(sta), clip(lta)


def _cft_host(a, type, nsta, nlta):
    return (_classic_host if type == "classicstalta" else _recursive_host)(_host_samples(a), nsta, nlta)


def trace_trigger(tr, type, sta, lta):
    """``tr.trigger(type, sta=..., lta=...)`` in place (``volpick_amd.Trace``): the data becomes the characteristic function.
    A device-backed trace stays on the device (float32); a host trace becomes float64, as in ObsPy."""
    if type not in TYPES:
        raise ValueError(f"trigger type {type!r} is not one of {sorted(TYPES)}")
    import torch

    nsta, nlta = _windows(tr, sta, lta)
    if nsta > nlta:
        raise ValueError(f"sta = {sta} s is longer than lta = {lta} s")
    return trace_in_place(tr, "STA/LTA", lambda dev: sta_lta_device(dev, type, nsta, nlta, torch.float32),
                          lambda a: _cft_host(a, type, nsta, nlta))


def sta_lta_triggers(stream, type="recstalta", sta=5.0, lta=20.0, thr_on=2.0, thr_off=0.5):
    """The reference's waveform check in one call: per trace id a dict ``on``, ``off``, ``peak`` (int64 samples), ``value``
    (float32, the characteristic function at ``peak``) and ``cft`` (the characteristic function: a float32 CUDA tensor for a
    device-backed trace, a float64 array for a host trace).  The stream is left alone.  Device-backed traces of equal length,
    kind, rate and device go through ONE ``vp_sta_lta`` call and ONE ``vp_trigger_onset`` call (where the library refuses --
    a window beyond its limit -- a warning says so and they take the host path, as in ``Trace.filter``); host traces through
    the host path, their triggers cut from the float32 rounding of their cft as on the device."""
    if type not in TYPES:
        raise ValueError(f"trigger type {type!r} is not one of {sorted(TYPES)}")
    import torch

    out, groups = {}, {}

    def on_host(tr):
        nsta, nlta = _windows(tr, sta, lta)
        cft = _cft_host(tr.data, type, nsta, nlta)
        on, off, pk, val = _pick_host(cft.astype(np.float32), float(thr_on), float(thr_off))
        out[tr.id] = dict(on=on, off=off, peak=pk, value=val, cft=cft)

    def on_device(trs):
        nsta, nlta = _windows(trs[0], sta, lta)
        cft = sta_lta_device(torch.stack([trace_samples(t) for t in trs]), type, nsta, nlta, torch.float32)
        return cft, trigger_onset_device(cft, float(thr_on), float(thr_off))

    for tr in stream:
        dev = trace_samples(tr)
        if dev is not None and len(tr) > 0:
            key = (str(dev.device), str(dev.dtype), int(dev.shape[0]), float(tr.stats.sampling_rate))
            groups.setdefault(key, []).append(tr)
        else:
            on_host(tr)
    for trs in groups.values():
        res = try_on_device(trs[0].id, "STA/LTA", lambda: on_device(trs), "STA/LTA and triggers")
        if res is None:  # the library refused (a window beyond its limit): these traces take the host path
            for tr in trs:
                on_host(tr)
            continue
        cft, (on, off, pk, val, ser) = res
        for k, tr in enumerate(trs):
            m = ser == k
            out[tr.id] = dict(on=on[m], off=off[m], peak=pk[m], value=val[m], cft=cft[k])
    return out


def release_trigger_scratch(device=0):
    """Free the scratch ``vp_sta_lta`` and ``vp_trigger_onset`` keep per device between calls; returns the bytes freed."""
    return release_scratch("vp_sta_lta_release_scratch", device)
