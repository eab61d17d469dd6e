"""Event waveform files -> a device-resident :class:`~volpick_amd.generate.WaveformBank`, without a sample visiting the host.

The reference turns its event miniSEED files into training arrays with ``convert_mseed_to_seisbench`` (its
volpick/data/convert.py:73-298), one file at a time on the host: ``obspy.read``, a resample where a rate is not 100 Hz,
``detrend("demean")``, two conditional ``trim``s, ``stream_to_array`` (:26-70), then onset samples, SNR and frequency index.
Here the files are decoded by one launch per sample kind (:func:`volpick_amd.io.read_many`), the host plans from the
headers alone which samples go where (:func:`plan_event`: a restatement of :152-220 and :26-66 that never reads a sample),
and one ``vp_bank_assemble`` call (csrc/assemble.hip) demeans, places, zero-fills, demeans the rows and rounds once to fp32
for every event at once.  The attributes come from the existing :func:`~volpick_amd.attributes.bank_attributes`, whose
host wait is the only one of the whole route.

Choices that rest on behaviour of ObsPy that is not available here to pin are named constants: the ``TRIM_*`` constants
of :mod:`volpick_amd.stream`, and below

* ``RESAMPLE_ONLY_DIFFERING`` -- the reference calls ``Stream.resample(100)`` on the whole stream as soon as one trace
  differs; here only the traces at another rate are converted (by :func:`volpick_amd.resample.resample_trace`, on the
  device for device-backed traces), a trace already at the rate is left as it is;
* ``TRIM_TIMES_AS_GIVEN`` -- every trace is cut at the nearest sample to the given times by its own clock
  (``Trace.trim``'s rule); no snapping of the times to the first trace's sample grid beforehand.

Out of scope: ``trace_has_spikes`` (a SeisBench function that is not available here and cannot be pinned), the HDF5 / CSV
writer, the random train / dev / test split, the Japan column set, and masked traces, which are refused as the other trace
operations refuse them.
"""
from __future__ import annotations

import math

import numpy as np

from ._device import SAMPLE_KINDS, device_backing, trace_samples
from .generate import ASSEMBLE_PIECE, WaveformBank
from .stream import Stream, UTCDateTime, to_device, trim_cut

RESAMPLE_ONLY_DIFFERING = True
TRIM_TIMES_AS_GIVEN = True

TABLE_COLUMNS = ("trace_start_time", "trace_npts", "trace_completeness", "trace_p_arrival_sample", "trace_s_arrival_sample",
                 "trace_sampling_rate_hz")


def _missing(t):
    """pd.isna for one arrival time: None, NaN, NaT."""
    return t is None or (isinstance(t, float) and math.isnan(t)) or t != t


class _Span:
    """One trace's header as the reference's steps change it: ``source`` (the trace the samples come from, at the common
    rate), its full length ``mean_n`` (what ``detrend("demean")`` averaged over), and the samples ``[first, first + npts)``
    of it that the trims have left, starting at ``starttime``."""

    __slots__ = ("source", "channel", "rate", "mean_n", "first", "npts", "starttime")

    def __init__(self, tr):
        self.source, self.channel, self.rate = tr, tr.stats.channel, float(tr.stats.sampling_rate)
        self.mean_n = self.npts = int(tr.stats.npts)
        self.first, self.starttime = 0, UTCDateTime(tr.stats.starttime)

    @property
    def endtime(self):
        return self.starttime + max(self.npts - 1, 0) / self.rate

    def trim(self, t_start, t_end):
        first, count = trim_cut(self.starttime, self.npts, self.rate, t_start, t_end)
        if first and count:
            self.starttime = self.starttime + first / self.rate
        self.first, self.npts = self.first + first, count


def _trim(spans, t_start, t_end):
    """``Stream.trim``: every span cut, the empty ones dropped."""
    assert TRIM_TIMES_AS_GIVEN
    for sp in spans:
        sp.trim(t_start, t_end)
    return [sp for sp in spans if sp.npts]


def _extent(spans, what):
    if not spans:
        raise ValueError(f"plan_event: no trace left {what} (the reference fails here: min() of an empty sequence)")
    return min(sp.starttime for sp in spans), max(sp.endtime for sp in spans)


def plan_event(stream, p_time, s_time, component_order="ZNE", sampling_rate=100, cut_bounds=None, check_long_traces=False,
               check_long_traces_limit=150):
    """What ``convert_mseed_to_seisbench`` does to one event's stream between ``read`` and the attributes
    (convert.py:152-220 with ``stream_to_array``, :26-66), planned from the headers: no sample is read.

    Returns a dict: ``pieces`` -- one per trace that reaches the array, in the order the reference writes them
    (components in ``component_order``; within one, ascending ``npts`` by a stable sort, so the longest is written last and
    wins, ties in stream order), each a dict ``source`` (the trace the samples come from), ``component``, ``mean_n`` (the
    source's full length: the range its own mean is taken over), ``keep_lo`` / ``keep_n`` (the samples of it that land in
    the array) and ``dst`` (where) -- ``samples``, ``starttime``, ``completeness``, ``trace_p_arrival_sample`` /
    ``trace_s_arrival_sample`` (floats, NaN = no pick) and ``sampling_rate``.  The float arithmetic is the reference's:
    ``int((t - starttime) * rate)`` truncates the float64 product, so an offset of 0.29 s at 100 Hz is sample 28."""
    from .resample import resample_trace

    rate = sampling_rate
    spans = []
    for tr in stream:
        if device_backing(tr) is None and np.ma.isMaskedArray(tr.data):  # (a device-backed trace has no mask)
            raise NotImplementedError("masked traces cannot be converted; split the stream at its gaps first")
        if tr.stats.sampling_rate != rate:  # :153-159
            assert RESAMPLE_ONLY_DIFFERING
            tr = resample_trace(tr, float(rate), copy=True, fourier_on_device=True)
        spans.append(_Span(tr))  # :162 detrend("demean"): the mean is over the trace as it is now
    t0, t1 = _extent(spans, "in the stream")
    if isinstance(cut_bounds, (int, float)) and (t1 - t0) > (3 * cut_bounds + 60):  # :167-173
        spans = _trim(spans, t0 + cut_bounds, t1 - cut_bounds)
    t0, t1 = _extent(spans, "after the cut_bounds trim")
    if check_long_traces and (t1 - t0) > check_long_traces_limit:  # :177-195
        arr = [UTCDateTime(t) for t in (p_time, s_time) if not _missing(t)]
        if not arr:
            raise ValueError("plan_event: check_long_traces needs a P or an S arrival time (the reference fails here: min() of "
                             "an empty sequence)")
        spans = _trim(spans, max(min(arr) - check_long_traces_limit / 2, t0), min(max(arr) + check_long_traces_limit / 2, t1))
    # stream_to_array, :40-66
    starttime, endtime = _extent(spans, "after the long-trace trim")
    array_rate = spans[0].rate
    samples = int((endtime - starttime) * array_rate) + 1
    pieces, completeness = [], 0.0
    for ci, c in enumerate(component_order):
        sel = [sp for sp in spans if sp.channel.endswith(c)]
        if len(sel) > 1:
            sel = sorted(sel, key=lambda sp: sp.npts)
        c_completeness = 0.0
        for sp in sel:
            start_sample = int((sp.starttime - starttime) * array_rate)
            n = min(sp.npts, samples - start_sample)
            assert start_sample >= 0 and n >= 1
            pieces.append(dict(source=sp.source, component=ci, mean_n=sp.mean_n, keep_lo=sp.first, keep_n=n, dst=start_sample))
            c_completeness += n
        completeness += min(1.0, c_completeness / samples)
    out = dict(pieces=pieces, samples=samples, starttime=starttime, completeness=completeness / len(component_order),
               sampling_rate=rate)
    for name, t in (("p", p_time), ("s", s_time)):  # :211-219
        out[f"trace_{name}_arrival_sample"] = (float("nan") if _missing(t)
                                               else float(int((UTCDateTime(t) - starttime) * rate)))
    return out


def piece_table(plans):
    """The :data:`~volpick_amd.generate.ASSEMBLE_PIECE` array of ``plans`` (event i is bank trace i) and the device tensors
    it points into.  Every source must be device-backed."""
    n = sum(len(pl["pieces"]) for pl in plans)
    table = np.zeros(n, ASSEMBLE_PIECE)
    sources, k = [], 0
    for i, pl in enumerate(plans):
        for pc in pl["pieces"]:
            dev = trace_samples(pc["source"])
            if dev is None:
                raise TypeError("piece_table: a source trace is not backed by an int32, float32 or float64 device array")
            dev = dev.contiguous()
            assert int(dev.shape[0]) == pc["mean_n"]
            sources.append(dev)
            table[k] = (dev.data_ptr(), pc["mean_n"], pc["keep_lo"], pc["keep_n"], pc["dst"], i, pc["component"],
                        SAMPLE_KINDS[str(dev.dtype)], 0)
            k += 1
    return table, sources


def bank_from_streams(streams, metadata, component_order="ZNE", sampling_rate=100, cut_bounds=None, check_long_traces=False,
                      check_long_traces_limit=150, attributes=False, device=0):
    """``(bank, table)``: one bank trace per event stream, assembled on the device by one ``vp_bank_assemble`` call.

    ``streams``: one Stream per event (host traces are uploaded first, device-backed ones used where they lie).
    ``metadata``: a DataFrame or a dict of arrays with ``trace_p_arrival_time`` and ``trace_s_arrival_time`` (None / NaN /
    NaT = no pick), one entry per stream; the bank's P and S onsets are the arrival samples.  ``table``: a dict of arrays
    with :data:`TABLE_COLUMNS`; with ``attributes=True`` also ``trace_snr_db``, ``trace_mean_snr_db``,
    ``trace_frequency_index`` (:func:`~volpick_amd.attributes.bank_attributes`) and ``source_frequency_index``, the mean of
    ``trace_frequency_index`` per ``metadata["source_id"]`` (convert.py:282-297; NaN everywhere unless every trace has a P
    or an S sample).  Nothing waits for the device but ``bank_attributes``."""
    if len(component_order) != 3:
        raise ValueError("a waveform bank holds three components")
    streams = list(streams)
    p_times, s_times = (np.asarray(metadata[k], dtype=object).reshape(-1) for k in ("trace_p_arrival_time",
                                                                                 "trace_s_arrival_time"))
    if not (len(p_times) == len(s_times) == len(streams)):
        raise ValueError(f"{len(streams)} streams, {len(p_times)} P and {len(s_times)} S arrival times")
    plans = []
    for st, p, s in zip(streams, p_times, s_times):
        if any(device_backing(tr) is None for tr in st):
            st = to_device(st if isinstance(st, Stream) else Stream(list(st)), device)
        plans.append(plan_event(st, p, s, component_order, sampling_rate, cut_bounds, check_long_traces,
                                check_long_traces_limit))
    pieces, sources = piece_table(plans)
    p_s = np.array([pl["trace_p_arrival_sample"] for pl in plans])
    s_s = np.array([pl["trace_s_arrival_sample"] for pl in plans])
    lengths = np.array([pl["samples"] for pl in plans], np.int64)
    bank = WaveformBank.from_pieces(pieces, lengths, {"P": p_s, "S": s_s}, device=device, sources=sources)
    table = {
        "trace_start_time": np.array([str(pl["starttime"]) for pl in plans]),
        "trace_npts": lengths,
        "trace_completeness": np.array([pl["completeness"] for pl in plans]),
        "trace_p_arrival_sample": p_s,
        "trace_s_arrival_sample": s_s,
        "trace_sampling_rate_hz": np.full(len(plans), sampling_rate),
    }
    if attributes:
        from .attributes import bank_attributes

        att = bank_attributes(bank, sampling_rate)
        for k in ("trace_snr_db", "trace_mean_snr_db", "trace_frequency_index"):
            table[k] = att[k]
        table["source_frequency_index"] = source_frequency_index(
            metadata["source_id"] if "source_id" in metadata else np.arange(len(plans)), att["trace_frequency_index"], p_s, s_s)
    return bank, table


def source_frequency_index(source_id, trace_fi, p_sample, s_sample):
    """convert.py:282-297: per trace, the mean ``trace_frequency_index`` of its ``source_id``'s traces -- NaN for every
    trace unless each has a P or an S arrival sample."""
    sid = np.asarray(source_id).reshape(-1)
    fi = np.asarray(trace_fi, np.float64)
    if not np.all(np.isfinite(p_sample) | np.isfinite(s_sample)):
        return np.full(len(fi), np.nan)
    _, inv = np.unique(sid, return_inverse=True)
    means = np.array([np.mean(fi[inv == g]) for g in range(inv.max() + 1)])
    return means[inv]


def bank_from_mseed(sources, metadata, device=0, **kw):
    """:func:`volpick_amd.io.read_many` (one decode launch per sample kind for all files), then
    :func:`bank_from_streams`; ``sources`` are the event miniSEED files (paths, bytes or file objects)."""
    from .io import read_many

    return bank_from_streams(read_many(sources, device=device, device_resident=True), metadata, device=device, **kw)
