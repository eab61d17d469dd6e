"""Minimal waveform containers with the ObsPy surface the picker API touches.

ObsPy is not a dependency of this package (it is absent from the build image).
``Stream``/``Trace``/``UTCDateTime`` below reproduce the attributes the
reference's usage reads (README.md:38-82, Final_models/demo.ipynb:242-327):
``trace.stats.{network,station,location,channel,starttime,sampling_rate,npts,
endtime,delta}``, ``trace.data``, ``trace.id``, ``trace.times(reftime=...)``,
``stream.select(channel=...)``, ``stream.copy()``, ``stream.merge()``,
iteration / indexing / ``len``.  Real ObsPy streams are accepted too (duck
typing); see ``models._group_stream``.
"""
from __future__ import annotations

import copy as _copy
import fnmatch
import math
from collections import namedtuple
from datetime import datetime, timedelta, timezone

import numpy as np

from ._device import device_backing, upload_samples

_EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)


def pinned_array(shape, dtype=np.float32):
    """A numpy array in page-locked host memory (it keeps the torch tensor that owns the pages alive).  Trace data that lives
    in such arrays is uploaded by DMA straight from the caller's pages -- no staging copy through the runtime's own pinned
    buffers -- and asynchronously, so ``classify()`` overlaps the upload of the next station with the current one's compute at
    the link's full rate.  (Page-locking costs ~0.1 ms per MB once: for buffers that are filled many times -- a reader's
    ring, a real-time feed -- not for arrays used once.)"""
    import torch

    return torch.empty(tuple(np.atleast_1d(shape)), dtype=getattr(torch, np.dtype(dtype).name)).pin_memory().numpy()


class UTCDateTime:
    """UTC time stamp with microsecond resolution (integer microseconds since the epoch)."""

    __slots__ = ("_us",)

    def __init__(self, value=0.0):
        if isinstance(value, UTCDateTime):
            self._us = value._us
        elif isinstance(value, (int, float, np.integer, np.floating)):
            self._us = int(round(float(value) * 1e6))
        elif isinstance(value, datetime):
            if value.tzinfo is None:
                value = value.replace(tzinfo=timezone.utc)
            d = value - _EPOCH
            self._us = (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds
        elif isinstance(value, str):
            s = value.strip().replace("Z", "")
            fmt = "%Y-%m-%dT%H:%M:%S.%f" if "." in s else "%Y-%m-%dT%H:%M:%S"
            if "T" not in s:
                fmt = fmt.replace("T", " ") if " " in s else "%Y-%m-%d"
            self.__init__(datetime.strptime(s, fmt))
        elif hasattr(value, "timestamp"):  # obspy.UTCDateTime
            ts = value.timestamp
            self._us = int(round(float(ts() if callable(ts) else ts) * 1e6))
        else:
            raise TypeError(f"cannot build UTCDateTime from {type(value)}")

    @classmethod
    def _from_us(cls, us):
        o = cls.__new__(cls)
        o._us = int(us)
        return o

    @property
    def timestamp(self) -> float:
        return self._us / 1e6

    @property
    def datetime(self) -> datetime:
        return _EPOCH + timedelta(microseconds=self._us)

    def __add__(self, seconds):
        return UTCDateTime._from_us(self._us + int(round(float(seconds) * 1e6)))

    __radd__ = __add__

    def __sub__(self, other):
        if isinstance(other, UTCDateTime):
            return (self._us - other._us) / 1e6
        if hasattr(other, "timestamp") and not isinstance(other, (int, float)):
            return self.timestamp - UTCDateTime(other).timestamp
        return UTCDateTime._from_us(self._us - int(round(float(other) * 1e6)))

    def _key(self, other):
        return UTCDateTime(other)._us

    def __eq__(self, other):
        try:
            return self._us == self._key(other)
        except TypeError:
            return NotImplemented

    def __lt__(self, other):
        return self._us < self._key(other)

    def __le__(self, other):
        return self._us <= self._key(other)

    def __gt__(self, other):
        return self._us > self._key(other)

    def __ge__(self, other):
        return self._us >= self._key(other)

    def __hash__(self):
        return hash(self._us)

    def __float__(self):
        return self.timestamp

    def __str__(self):
        return self.datetime.strftime("%Y-%m-%dT%H:%M:%S.%f") + "Z"

    def __repr__(self):
        return f"UTCDateTime({str(self)!r})"


# --- station blocks: which samples of a stream form one (C, N) array.  ``plan_blocks`` is the only statement of the rule;
# ``models._group_stream`` fills its blocks with the samples of traces and ``io.plan_file_blocks`` with miniSEED records, so
# the two cannot disagree by a sample or a microsecond
def sample_offset(start, origin, sampling_rate):
    """The sample number of the time ``start`` in a block that begins at ``origin`` (both ``UTCDateTime``)."""
    return int(round((start - origin) * sampling_rate))


def block_start(origin, first_sample, sampling_rate):
    """The start time of the block that begins ``first_sample`` samples after ``origin``."""
    return origin + first_sample / sampling_rate


COMPONENT_ALIAS = {"1": "N", "2": "E", "3": "Z"}  # flexible horizontal components


def component_index(channel, component_order):
    """The row of ``channel``'s component in a block ordered as ``component_order``; -1: the block has no row for it."""
    comp = channel[-1] if channel else ""
    comp = comp if comp in component_order else COMPONENT_ALIAS.get(comp, comp)
    return component_order.index(comp) if comp in component_order else -1


def warn_short_fragment():
    import warnings

    warnings.warn("Parts of the input stream consist of fragments shorter than the number of input "
                  "samples. Output might be empty.")


BlockRun = namedtuple("BlockRun", "network station location t_start b0 b1 short pieces used")


def plan_blocks(pieces, component_order, sampling_rate, in_samples):
    """The station blocks of a stream, from headers alone: one ``BlockRun`` per contiguous run of one instrument, instruments
    in sorted order, an instrument's runs ascending.  ``pieces``, in stream order: ``(network, station, location, channel,
    start, npts, ref)`` with ``start`` a ``UTCDateTime`` and ``ref`` whatever the caller needs to find the samples again.

    An instrument is ``(network, station, location, channel[:-1])``; its origin ``t_start`` is the earliest start of its
    pieces, empty ones included.  A piece becomes ``(s0, npts, row, ref)``: first sample after the origin, length, component
    row or -1 (the block has no row for it).  Runs are the union of ``[s0, s0 + npts)`` over the pieces with samples, of
    every component, known or not; abutting pieces merge, gaps are not bridged.  The run covers samples ``[b0, b1)`` and
    starts at ``block_start(t_start, b0, sampling_rate)``; ``short``: it has fewer than ``in_samples`` samples, and what to do
    about it is the caller's.  ``pieces``: all of the instrument's; ``used``: those with a row that reach into the run; both
    in stream order (the assembly's "among equally long traces the later one wins" depends on it)."""
    groups = {}
    for net, sta, loc, cha, start, npts, ref in pieces:
        groups.setdefault((net, sta, loc, cha[:-1]), []).append((cha, start, npts, ref))
    for (net, sta, loc, _), members in sorted(groups.items(), key=lambda g: g[0]):
        t_start = min(m[1] for m in members)
        placed = [(sample_offset(start, t_start, sampling_rate), npts, component_index(cha, component_order), ref)
                  for cha, start, npts, ref in members]
        runs = []
        for s0, npts, _, _ in sorted(placed, key=lambda p: p[0]):
            if npts <= 0:
                continue
            if runs and s0 <= runs[-1][1]:
                runs[-1][1] = max(runs[-1][1], s0 + npts)
            else:
                runs.append([s0, s0 + npts])
        for b0, b1 in runs:
            used = [p for p in placed if p[2] >= 0 and min(p[0] + p[1], b1) > max(p[0], b0)]
            yield BlockRun(net, sta, loc, t_start, b0, b1, b1 - b0 < in_samples, placed, used)


def block_dict(data, network, station, location, starttime):
    """One station block as ``classify`` / ``annotate`` take it: ``data`` (C, N), its start and whose it is."""
    return {"data": data, "starttime": starttime, "trace_id": f"{network}.{station}.{location}", "network": network,
            "station": station, "location": location}


# --- ObsPy's Trace.trim(starttime, endtime) with its defaults, restated (ObsPy is not available to pin it) ------------------
TRIM_PAD = False              # pad=False: a time outside the trace cuts nothing, it never adds samples
TRIM_NEAREST_SAMPLE = True    # nearest_sample=True: the cut lands on the sample nearest to the given time ...
TRIM_ROUNDING = "half_away"   # ... by ObsPy's round_away: halves go away from zero (2.5 -> 3, -2.5 -> -3), not to even


def round_half_away(x):
    """The integer nearest to ``x``, halves away from zero (ObsPy's ``compatibility.round_away``)."""
    assert TRIM_ROUNDING == "half_away"
    x = float(x)
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def trim_cut(starttime, npts, rate, t_start=None, t_end=None):
    """``(first, count)``: the samples ``[first, first + count)`` of a trace of ``npts`` samples at ``rate`` Hz from
    ``starttime`` that ``trim(t_start, t_end)`` keeps.  Left: ``delta = round_half_away((t_start - starttime) * rate)``, a
    cut only when ``delta > 0``.  Right, on the trace the left cut has left: ``delta = round_half_away((t_end - its start)
    * rate) - its npts + 1``, a cut only when ``delta < 0``.  An end before the start leaves nothing."""
    assert TRIM_NEAREST_SAMPLE and not TRIM_PAD
    starttime = UTCDateTime(starttime)
    if t_start is not None and t_end is not None and UTCDateTime(t_start) > UTCDateTime(t_end):
        return 0, 0
    first, count = 0, int(npts)
    if t_start is not None:
        delta = round_half_away((UTCDateTime(t_start) - starttime) * rate)
        if delta > 0:
            first = min(delta, count)
            count -= first
            if count:
                starttime = starttime + first / rate
    if t_end is not None and count:
        delta = round_half_away((UTCDateTime(t_end) - starttime) * rate) - count + 1
        if delta < 0:
            count = max(count + delta, 0)
    return first, count


def _write(stream_or_trace, target, format, kw):
    if str(format).upper() != "MSEED":
        raise ValueError(f"unsupported output format {format!r} (MSEED is implemented)")
    from .io import write_mseed

    return write_mseed(stream_or_trace, target, **kw)


class Stats(dict):
    """Trace header; attribute and item access, derived npts / delta / endtime."""

    _defaults = dict(network="", station="", location="", channel="", starttime=None, sampling_rate=1.0, npts=0)

    def __init__(self, header=None):
        super().__init__(self._defaults)
        self["starttime"] = UTCDateTime(0)
        if header:
            for k, v in dict(header).items():
                self[k] = v

    def __setitem__(self, k, v):
        if k == "starttime":
            v = UTCDateTime(v)
        elif k == "sampling_rate":
            v = float(v)
        super().__setitem__(k, v)

    def __getattr__(self, k):
        if k == "delta":
            return 1.0 / self["sampling_rate"]
        if k == "endtime":
            return self["starttime"] + max(self["npts"] - 1, 0) / self["sampling_rate"]
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def copy(self):
        return Stats(dict(self))


class Trace:
    """``data`` is a numpy array.  A trace may instead be backed by a device array (``device_data``: a CUDA
    torch tensor, as ``volpick_amd.read(..., device_resident=True)`` produces); ``data`` then materialises a
    host copy on first access, and the picker consumes the device array directly."""

    def __init__(self, data=None, header=None, device_data=None):
        self._dev = device_data
        if data is None and device_data is not None:
            self._data = None
            n = int(device_data.shape[0])
        else:
            # (asanyarray: a masked array -- what a gappy merge leaves -- keeps its mask, as in an ObsPy trace)
            self._data = np.asanyarray(data if data is not None else np.zeros(0, dtype=np.float32))
            n = len(self._data)
        self.stats = Stats(header)
        self.stats["npts"] = n

    @property
    def data(self):
        if self._data is None:
            self._data = self._dev.cpu().numpy()
        return self._data

    @data.setter
    def data(self, value):
        self._data = np.asanyarray(value)
        self._dev = None
        self.stats["npts"] = len(self._data)

    @property
    def id(self):
        s = self.stats
        return f"{s.network}.{s.station}.{s.location}.{s.channel}"

    def times(self, type="relative", reftime=None):
        t = np.arange(len(self.data)) / self.stats.sampling_rate
        if reftime is not None:
            t = t + (self.stats.starttime - UTCDateTime(reftime))
        return t

    def copy(self):
        return Trace(self.data.copy(), self.stats.copy())

    def trim(self, starttime=None, endtime=None):
        """ObsPy's ``Trace.trim(starttime, endtime)`` with its defaults ``pad=False, nearest_sample=True``, in place; returns
        ``self``.  A restatement of ObsPy's rule (:func:`trim_cut` and the ``TRIM_*`` constants beside it), not ObsPy's code.
        A device-backed trace is cut by slicing its tensor -- a view of the same storage, no copy, no host visit -- a host
        trace by slicing its array."""
        first, count = trim_cut(self.stats.starttime, self.stats.npts, self.stats.sampling_rate, starttime, endtime)
        if first == 0 and count == self.stats.npts:
            return self
        if self._dev is not None:
            self._dev = self._dev[first:first + count]
            if self._data is not None:
                self._data = self._data[first:first + count]
        else:
            self._data = self._data[first:first + count]
        if first and count:
            self.stats["starttime"] = self.stats.starttime + first / self.stats.sampling_rate
        self.stats["npts"] = count
        return self

    def filter(self, type, **options):
        """ObsPy's ``Trace.filter``: ``lowpass`` / ``highpass`` (``freq``), ``bandpass`` / ``bandstop`` (``freqmin``,
        ``freqmax``); ``corners=4``, ``zerophase=False``.  In place, returns ``self``.  A device-backed trace is filtered on the
        device (float64 state, float32 samples) and stays there; a host trace becomes float64, as in ObsPy."""
        from .signal import filter_trace

        return filter_trace(self, type, **options)

    def detrend(self, type="simple"):
        """ObsPy's ``Trace.detrend`` for ``simple``, ``linear``, ``demean`` / ``constant``.  In place, returns ``self``; device-backed
        traces on the device, as :meth:`filter`."""
        from .signal import detrend_trace

        return detrend_trace(self, type)

    def spectrogram(self, **kw):
        """The numbers of a spectrogram, on the GPU: ObsPy's method of this name draws; this one returns what it would draw --
        a ``volpick_amd.spectrogram.Spectrogram`` ``(data, freq, time)``, ``data`` a float32 CUDA tensor ``(n_freq, n_frames)``
        as the reference's ``specgram[f, t]``.  Keywords: ``per_lap=0.9, wlen=None, dbscale=False, mult=8.0, frames=None`` (see
        ``volpick_amd.spectrogram.spectrogram``).  A device-backed trace is read where it lies and stays there; a host trace is
        uploaded and goes through the same kernel (no host fallback); a masked trace is refused."""
        from .spectrogram import trace_spectrogram

        return trace_spectrogram(self, **kw)

    def trigger(self, type, sta, lta):
        """ObsPy's ``Trace.trigger`` for ``classicstalta`` and ``recstalta``: the data becomes the STA/LTA characteristic
        function, ``sta`` and ``lta`` in seconds (``int(seconds * sampling_rate)`` samples, clipped to ``[1, npts]``).  In
        place, returns ``self``.  A device-backed trace is processed on the device (float64 arithmetic, float32 samples) and
        stays there; a host trace becomes float64."""
        from .trigger import trace_trigger

        return trace_trigger(self, type, sta, lta)

    def write(self, target, format="MSEED", **kw):
        """ObsPy's ``Trace.write`` for miniSEED: ``volpick_amd.io.write_mseed(self, target, **kw)``.  A device-backed trace is
        packed from where it lies; any other ``format`` is refused."""
        return _write(self, target, format, kw)

    def __len__(self):
        return int(self.stats["npts"])

    def __str__(self):
        s = self.stats
        return f"{self.id} | {s.starttime} - {s.endtime} | {s.sampling_rate:.1f} Hz, {len(self)} samples"

    __repr__ = __str__


class Stream:
    def __init__(self, traces=None):
        self.traces = list(traces) if traces is not None else []

    def __iter__(self):
        return iter(self.traces)

    def __len__(self):
        return len(self.traces)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return Stream(self.traces[i])
        return self.traces[i]

    def __add__(self, other):
        return Stream(self.traces + list(other))

    def __iadd__(self, other):
        self.traces.extend(list(other))
        return self

    def append(self, tr):
        self.traces.append(tr)
        return self

    def copy(self):
        return Stream([t.copy() for t in self.traces])

    def trim(self, starttime=None, endtime=None):
        """``Trace.trim`` on every trace, in place; traces left empty are dropped, as ObsPy's ``Stream.trim`` does."""
        for tr in self.traces:
            tr.trim(starttime, endtime)
        self.traces = [tr for tr in self.traces if tr.stats.npts]
        return self

    def filter(self, type, **options):
        for tr in self.traces:
            tr.filter(type, **options)
        return self

    def detrend(self, type="simple"):
        for tr in self.traces:
            tr.detrend(type)
        return self

    def spectrogram(self, **kw):
        """``[tr.spectrogram(**kw) for tr in self]``: one result per trace (ObsPy's method draws; this one returns numbers)."""
        return [tr.spectrogram(**kw) for tr in self.traces]

    def trigger(self, type, sta, lta):
        for tr in self.traces:
            tr.trigger(type, sta=sta, lta=lta)
        return self

    def write(self, target, format="MSEED", **kw):
        """ObsPy's ``Stream.write`` for miniSEED: ``volpick_amd.io.write_mseed(self, target, **kw)``, the traces in stream order
        through one set of launches; any other ``format`` is refused."""
        return _write(self, target, format, kw)

    def sort(self, keys=("network", "station", "location", "channel", "starttime")):
        self.traces.sort(key=lambda t: tuple(str(t.stats[k]) if k != "starttime" else t.stats[k]._us for k in keys))
        return self

    def select(self, network=None, station=None, location=None, channel=None, component=None, id=None):
        out = []
        for tr in self.traces:
            s = tr.stats
            if network is not None and not fnmatch.fnmatchcase(s.network, network):
                continue
            if station is not None and not fnmatch.fnmatchcase(s.station, station):
                continue
            if location is not None and not fnmatch.fnmatchcase(s.location, location):
                continue
            if channel is not None and not fnmatch.fnmatchcase(s.channel, channel):
                continue
            if component is not None and not (s.channel and fnmatch.fnmatchcase(s.channel[-1], component)):
                continue
            if id is not None and not fnmatch.fnmatchcase(tr.id, id):
                continue
            out.append(tr)
        return Stream(out)

    def merge(self, method=0, fill_value=None):
        """Join traces of the same id.  ``method=-1`` (the clean-up merge annotate() performs)
        only joins exactly contiguous / duplicate-free pieces; other methods additionally fill
        gaps with ``fill_value`` (0 if None).  Overlaps keep the earlier trace's samples."""
        groups = {}
        for tr in self.traces:
            groups.setdefault((tr.id, tr.stats.sampling_rate), []).append(tr)
        merged = []
        for (_, sr), trs in groups.items():
            trs.sort(key=lambda t: t.stats.starttime._us)
            cur = trs[0].copy()
            for nxt in trs[1:]:
                expected = cur.stats.starttime + len(cur.data) / sr
                gap = int(round((nxt.stats.starttime - expected) * sr))
                if gap == 0:
                    cur.data = np.concatenate([cur.data, nxt.data])
                elif gap > 0 and method != -1:
                    fill = np.full(gap, 0 if fill_value is None else fill_value, dtype=cur.data.dtype)
                    cur.data = np.concatenate([cur.data, fill, nxt.data])
                elif gap < 0 and method != -1:
                    keep = nxt.data[-gap:] if -gap < len(nxt.data) else nxt.data[:0]
                    cur.data = np.concatenate([cur.data, keep])
                else:
                    cur.stats["npts"] = len(cur.data)
                    merged.append(cur)
                    cur = nxt.copy()
                    continue
            cur.stats["npts"] = len(cur.data)
            merged.append(cur)
        self.traces = merged
        return self

    def __str__(self):
        return f"{len(self.traces)} Trace(s) in Stream:\n" + "\n".join(str(t) for t in self.traces)

    __repr__ = __str__


def to_device(stream, device=0):
    """A new Stream whose traces are device-backed: every trace's samples uploaded to ``cuda:device`` in their own dtype (int32,
    float32, float64; anything else as float32), headers copied.  ``classify`` / ``annotate`` then assemble, and where the
    rate differs from the model's decimate or Fourier-resample, on the GPU.  Traces that already live on that device are shared,
    not copied; masked traces are refused (split the stream at its gaps first)."""
    import torch

    dev = torch.device("cuda", int(device))
    out = Stream()
    for tr in stream:
        d = device_backing(tr)
        if d is None:
            d = upload_samples(tr.data, dev, "masked traces cannot be moved to the device")
        elif d.device != dev:
            d = d.to(dev)
        hdr = Stats({k: v for k, v in dict(tr.stats).items() if k not in ("npts", "delta", "endtime")})
        hdr["starttime"] = UTCDateTime(tr.stats.starttime)
        out.append(Trace(header=hdr, device_data=d))
    return out


def deepcopy_stream(stream):
    return stream.copy() if hasattr(stream, "copy") else _copy.deepcopy(stream)


__all__ = ["UTCDateTime", "Stats", "Trace", "Stream", "math"]
