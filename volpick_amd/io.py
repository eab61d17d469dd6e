"""Waveform-file ingestion without ObsPy.

``read()`` stands where the reference calls ``obspy.read`` ahead of the picker
(the reference's volpick/data/convert.py:7 and the ``read(...)`` call sites of
``convert_mseed_to_seisbench``; Final_models/demo.ipynb:249-266 builds the same kind of Stream
from an FDSN download) and returns this package's ``Stream``.  miniSEED 2 and miniSEED 3 records
(also mixed in one file) are found by the library's host scanner (``vp_mseed_scan``, which checks
the CRC-32C of miniSEED 3 records) and unpacked on the GPU (``vp_mseed_decode``: one wavefront per
record, Steim-1/2, the plain 16 / 24 / 32-bit integer and float encodings, text); there is no CPU
decoder in the product -- without a GPU ``read`` of a miniSEED file raises.  SAC files are a
header plus raw float32 samples and need no kernel.

``stream_to_array`` is the array-assembly rule of volpick/data/convert.py:26-70.

``write_mseed()`` is the other direction, the reference's ``waveforms.write(path, format="MSEED")``
(volpick/data/data.py:1353): miniSEED 2 records packed on the GPU (``vp_mseed_encode``: Steim-1/2 and the plain
encodings), headers built by the library on the host; no host encoder either.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import threading
from datetime import datetime, timedelta, timezone

import numpy as np

from . import _lib
from ._device import device_backing, release_scratch, upload_samples
from .stream import Stream, Trace, UTCDateTime, block_start, plan_blocks, warn_short_fragment

_REC_DTYPE = np.dtype(
    [("offset", "<i8"), ("start_us", "<i8"), ("sample_rate", "<f8"), ("reclen", "<i4"), ("data_offset", "<i4"),
     ("nsamples", "<i4"), ("encoding", "<i4"), ("big_endian", "<i4"), ("quality", "<i4"), ("network", "S4"),
     ("station", "S8"), ("location", "S4"), ("channel", "S4")], align=True)
assert _REC_DTYPE.itemsize == C.sizeof(_lib.VpMseedRecord)
_FLOAT_ENCODINGS = (4, 5)
_EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)


def _as_bytes(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if hasattr(source, "read"):
        return source.read()
    with open(os.fspath(source), "rb") as f:
        return f.read()


def _looks_like_mseed(buf):
    h = buf[:8]
    if h[:3] == b"MS\x03":
        return True
    return len(h) >= 8 and all(48 <= c <= 57 or c == 32 for c in h[:6]) and h[6:7] in (b"D", b"R", b"Q", b"M")


def _scan_to_fit(buf, scan):
    """``scan(cap)`` -> ``(result, records found)`` with a table of ``cap`` records, again with room for all of them if the
    first table was too small; returns the result.  The first capacity comes from the first record's length (miniSEED 2:
    2 ** byte 6 of blockette 1000, usually at byte 48 + 6; miniSEED 3 records vary) -- a table sized for 256-byte records is
    10 MB of zeroed ctypes memory for a 35 MB station-day of 4096-byte records; the scanner reports the real count, so a low
    guess costs one more pass."""
    guess = 512
    if len(buf) >= 56 and buf[:3] != b"MS\x03" and buf[48:50] in (b"\x03\xe8", b"\xe8\x03") and 7 <= buf[54] <= 24:
        guess = 1 << buf[54]
    cap = max(16, len(buf) // guess + 16)
    while True:
        result, found = scan(cap)
        if found <= cap:
            return result
        cap = found


def scan_mseed(buf):
    """Record table of a miniSEED byte string as a numpy structured array (host only)."""
    lib = _lib.load()
    n = C.c_int64(0)

    def scan(cap):
        recs = (_lib.VpMseedRecord * cap)()
        _lib.check(lib.vp_mseed_scan(buf, len(buf), recs, cap, C.byref(n)), "vp_mseed_scan")
        return recs, n.value

    return np.frombuffer(_scan_to_fit(buf, scan), dtype=_REC_DTYPE, count=n.value).copy()


def _segments(recs):
    """Order records by (source id, start time) and chain them into continuous segments: a record
    extends the previous one of the same id, rate and sample kind when it starts one sample period
    after that record's last sample, within half a period (libmseed trace-list tolerance)."""
    order = np.lexsort((recs["offset"], recs["start_us"], recs["channel"], recs["location"], recs["station"],
                        recs["network"]))
    keep = order if (recs["nsamples"] > 0).all() else order[recs["nsamples"][order] > 0]
    # (rows of bytes: fancy indexing of a structured array copies field by field -- 1.9 of this function's 2.9 ms per station-day)
    rows = np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), recs.dtype.itemsize)
    r = rows[keep].view(recs.dtype).reshape(-1)
    if len(r) == 0:
        return r, np.zeros(0, np.int64)
    period = np.where(r["sample_rate"] > 0, 1e6 / np.where(r["sample_rate"] > 0, r["sample_rate"], 1.0), 0.0)
    is_float = np.isin(r["encoding"], _FLOAT_ENCODINGS)
    expect = r["start_us"][:-1] + np.round(r["nsamples"][:-1] * period[:-1]).astype(np.int64)
    same = np.ones(len(r) - 1, bool)
    for f in ("network", "station", "location", "channel", "sample_rate"):
        same &= r[f][1:] == r[f][:-1]
    same &= is_float[1:] == is_float[:-1]
    same &= np.abs(r["start_us"][1:] - expect) <= 0.5 * period[:-1]
    seg = np.concatenate([[0], np.cumsum(~same)]).astype(np.int64)
    return r, seg


def scan_segments(buf):
    """``_segments(scan_mseed(buf))`` in one host-only library call (``vp_mseed_scan_segments``): the ordered record table and
    the segment number of each record.  Touches no GPU and no handle: any thread may call it."""
    lib = _lib.load()
    n, kept = C.c_int64(0), C.c_int64(0)

    def scan(cap):
        recs, seg = np.empty(cap, _REC_DTYPE), np.empty(cap, np.int64)
        _lib.check(lib.vp_mseed_scan_segments(buf, len(buf), recs.ctypes.data_as(C.POINTER(_lib.VpMseedRecord)),
                                              seg.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n), C.byref(kept)),
                   "vp_mseed_scan_segments")
        return (recs, seg), n.value

    recs, seg = _scan_to_fit(buf, scan)
    return recs[:kept.value], seg[:kept.value]


class FilePlan:
    """What :func:`plan_file_blocks` found.  ``reason`` is ``None`` when the file can be decoded straight into its station
    blocks, else why not (the file then goes through :func:`read_mseed`).  ``blocks``: one dict per block, in the order
    ``models._group_stream`` yields them -- ``trace_id``, ``network``, ``station``, ``location``, ``start_us``, ``shape``
    ``(C, N)`` and ``offset``, where the block begins in the file's float32 sample array (-1: no record feeds the block, it
    is all zeros).  ``out_index[r]``: where record ``r``'s first sample goes in that array, -1 for a record of no block.
    ``n_out``: the array's length.  ``short_runs``: how many runs were skipped as shorter than the model's window."""

    __slots__ = ("reason", "blocks", "out_index", "n_out", "short_runs")

    def __init__(self, reason=None, blocks=(), out_index=None, n_out=0, short_runs=0):
        self.reason, self.blocks, self.out_index, self.n_out, self.short_runs = reason, list(blocks), out_index, n_out, short_runs


BLOCK_ALIGN = 64  # blocks start on 256-byte boundaries of the file's sample array


def plan_file_blocks(table, seg, component_order, sampling_rate, in_samples, has_filter=False, warn=True):
    """From the headers alone, the station blocks of a miniSEED file and where every record's samples go in them, so that one
    decode launch (``vp_mseed_decode_on`` with float32 output and zero fill) writes the blocks ``models._group_stream`` would
    assemble from the traces of ``read(..., device_resident=True)``.  ``table`` and ``seg`` are :func:`scan_segments`'.  Every
    segment is a piece of ``stream.plan_blocks``, the planner ``_group_stream`` asks too: instruments, component rows, sample
    offsets, runs, used pieces and start times are its answers, and only ``out_index`` is worked out here.

    No plan (``FilePlan.reason`` set) when the file has no records; the model filters its input (``has_filter``); a trace is
    not at the model's rate (any trace: a resampled one changes length, and with it the runs); two segments of one component
    overlap inside a block (the assembly's "longer trace wins" is not a per-record rule); or a text record (encoding 0)
    belongs to a used component.  ``warn=False`` leaves the short-fragment warnings to the caller (``short_runs`` of them)."""
    if len(table) == 0:
        return FilePlan("no records")
    if has_filter:
        return FilePlan("the model filters its input")
    first, last = _segment_ranges(seg)
    if (np.abs(table["sample_rate"][first] - float(sampling_rate)) > 1e-6).any():
        return FilePlan("a trace is not at the model's rate")
    ns = table["nsamples"].astype(np.int64)
    before = np.cumsum(ns) - ns  # samples ahead of each record in the table
    code = lambda field, a: table[field][a].decode()  # noqa: E731
    pieces = [(code("network", a), code("station", a), code("location", a), code("channel", a),
               UTCDateTime._from_us(int(table["start_us"][a])), int(before[b - 1] + ns[b - 1] - before[a]), (a, b))
              for a, b in zip(first.tolist(), last.tolist())]  # a segment's ``ref`` is its records [a, b)
    plan = FilePlan(out_index=np.full(len(table), -1, np.int64))
    n_rows, cursor = len(component_order), 0
    for run in plan_blocks(pieces, component_order, sampling_rate, in_samples):
        if run.short:
            plan.short_runs += 1
            if warn:
                warn_short_fragment()
            continue
        used = sorted(run.used, key=lambda p: (p[2], p[0]))
        for p, q in zip(used, used[1:]):
            if p[2] == q[2] and q[0] < p[0] + p[1]:
                return FilePlan("two segments of one component overlap")
        if any(int(table["encoding"][a]) == 0 for _, _, _, (a, _) in used):
            return FilePlan("a text record belongs to a used component")
        n = run.b1 - run.b0
        plan.blocks.append(dict(trace_id=f"{run.network}.{run.station}.{run.location}", network=run.network,
                                station=run.station, location=run.location,
                                start_us=block_start(run.t_start, run.b0, sampling_rate)._us, shape=(n_rows, n),
                                offset=cursor if used else -1))
        for s0, _, row, (a, b) in used:
            plan.out_index[a:b] = cursor + row * n + (s0 - run.b0) + (before[a:b] - before[a])
        if used:
            cursor += -(-n_rows * n // BLOCK_ALIGN) * BLOCK_ALIGN
    plan.n_out = cursor
    return plan


def _decode(buf, r, bounds, bases, device, dtype, device_resident):
    """The samples of the record table ``r`` (as :func:`_segments` orders it) of the bytes ``buf``, by one ``vp_mseed_decode``
    per sample kind the table holds.  Returns ``(as_float, buffers)``: which records were decoded to float32 (the float
    encodings; every record when ``dtype`` is float32), and per kind ``(out, index, status)`` -- the samples record after
    record in a numpy array or, with ``device_resident``, a CUDA tensor; where each record starts in it; the decoder's status
    per record.  ``bounds`` and ``bases`` are :func:`many_tables`' (one file: ``[0, len(r)]`` and ``[0]``): they name the file
    of a short payload."""
    lib = _lib.load()
    as_float = np.isin(r["encoding"], _FLOAT_ENCODINGS) | (dtype is not None and np.dtype(dtype) == np.float32)
    recs_c = (_lib.VpMseedRecord * len(r)).from_buffer_copy(np.ascontiguousarray(r).tobytes())
    buffers = {}
    for kind, sel in ((_lib.VP_SAMPLES_INT32, ~as_float), (_lib.VP_SAMPLES_FLOAT32, as_float)):
        if not sel.any():
            continue
        ns = np.where(sel, r["nsamples"], 0).astype(np.int64)
        index = np.where(sel, np.cumsum(ns) - ns, -1).astype(np.int64)
        n_out = int(ns.sum())
        status = np.zeros(len(r), np.int32)
        if device_resident:
            import torch

            out = torch.empty(n_out, dtype=torch.int32 if kind == _lib.VP_SAMPLES_INT32 else torch.float32,
                              device=torch.device("cuda", device))
            out_ptr, out_mem = C.c_void_p(out.data_ptr()), _lib.VP_MEM_DEVICE
        else:
            out = np.empty(n_out, dtype=np.int32 if kind == _lib.VP_SAMPLES_INT32 else np.float32)
            out_ptr, out_mem = out.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST
        _lib.check(
            lib.vp_mseed_decode(device, buf, _lib.VP_MEM_HOST, len(buf), recs_c,
                                index.ctypes.data_as(C.POINTER(C.c_int64)), None, len(r), kind,
                                out_ptr, out_mem, n_out, 0,
                                status.ctypes.data_as(C.POINTER(C.c_int32))), "vp_mseed_decode")
        err = short_payload_error(r, status, bounds, bases)
        if err is not None:
            raise err
        buffers[kind] = (out, index, status)
    return as_float, buffers


def _segment_ranges(seg):
    """``(first, last)``: segment ``i`` of the numbering ``seg`` (non-empty) is the records ``[first[i], last[i])``."""
    first = np.flatnonzero(np.concatenate([[True], seg[1:] != seg[:-1]]))
    return first, np.concatenate([first[1:], [len(seg)]])


def _add_traces(st, r, first, last, decoded, dtype, device_resident):
    """One ``Trace`` per segment ``[first[i], last[i])`` of the table ``r``, appended to ``st``; ``decoded`` is what
    :func:`_decode` returned for ``r``.  The traces are views into its buffers, except where a host trace is cast."""
    as_float, buffers = decoded
    for a, b in zip(first, last):
        kind = _lib.VP_SAMPLES_FLOAT32 if as_float[a] else _lib.VP_SAMPLES_INT32
        out, index, status = buffers[kind]
        n = int(r["nsamples"][a:b].sum())
        data = out[index[a]:index[a] + n]
        if device_resident:
            tr_args = dict(device_data=data)
        else:
            if dtype is not None and data.dtype != np.dtype(dtype):
                data = data.astype(dtype)
            elif int(r["encoding"][a]) == 0 and dtype is None:
                data = data.astype(np.uint8).view("S1")
            tr_args = dict(data=data)
        tr = Trace(header=dict(network=r["network"][a].decode(), station=r["station"][a].decode(),
                              location=r["location"][a].decode(), channel=r["channel"][a].decode(),
                              starttime=UTCDateTime._from_us(int(r["start_us"][a])),
                              sampling_rate=float(r["sample_rate"][a])), **tr_args)
        q = int(r["quality"][a])
        tr.stats["mseed"] = dict(dataquality=chr(q) if q < 256 else "", format_version=2 if q < 256 else 3,
                                 publication_version=q & 255 if q >= 256 else None, number_of_records=int(b - a),
                                 encoding=int(r["encoding"][a]), byteorder=">" if r["big_endian"][a] else "<",
                                 record_length=int(r["reclen"][a]),
                                 steim_integrity_errors=int((status[a:b] == 1).sum()))
        tr.stats["_format"] = "MSEED"
        st.append(tr)


def read_mseed(source, device=0, dtype=None, device_resident=False):
    """miniSEED -> Stream (one Trace per continuous segment, sorted by id and time).

    Integer encodings decode to int32 exactly; float32/float64 records to float32; text records
    (encoding 0: log channels) to ObsPy's ``|S1`` characters.  ``dtype`` forces the sample type of
    every trace (``np.float32`` decodes integers straight to fp32).
    ``device_resident=True`` leaves the decoded samples on the GPU: the traces are backed by CUDA
    tensors, ``classify`` / ``annotate`` assemble and consume them there, and ``trace.data`` copies
    to the host only when somebody reads it.

    The one-file case of :func:`read_many`, without its table and byte concatenation.
    """
    buf = _as_bytes(source)
    r, seg = _segments(scan_mseed(buf))
    st = Stream()
    if len(r):
        decoded = _decode(buf, r, (0, len(r)), (0,), device, dtype, device_resident)
        _add_traces(st, r, *_segment_ranges(seg), decoded, dtype, device_resident)
    return st


def many_tables(bufs):
    """Host bookkeeping of :func:`read_many`: ``(table, seg, bounds, bases)``.  ``table`` holds every file's records as
    :func:`_segments` orders them, file after file, with ``offset`` shifted by the file's position ``bases[k]`` in the
    concatenated bytes; ``seg`` numbers the continuous segments, which never reach across a file boundary (each file is
    scanned and chained on its own, and its segment numbers start behind the previous file's); file ``k`` owns the records
    ``[bounds[k], bounds[k + 1])``."""
    tables, segs, bounds, bases = [], [], [0], []
    pos = next_seg = 0
    for buf in bufs:
        r, seg = _segments(scan_mseed(buf))
        r = r.copy()
        r["offset"] += pos
        tables.append(r)
        segs.append(seg + next_seg)
        if len(seg):
            next_seg += int(seg[-1]) + 1
        bounds.append(bounds[-1] + len(r))
        bases.append(pos)
        pos += len(buf)
    table = np.concatenate(tables) if tables else np.zeros(0, _REC_DTYPE)
    seg = np.concatenate(segs) if segs else np.zeros(0, np.int64)
    return table, seg, np.asarray(bounds, np.int64), np.asarray(bases, np.int64)


def short_payload_error(table, status, bounds, bases):
    """The ``ValueError`` :func:`read_mseed` and :func:`read_many` raise for the first record (in table order) whose payload is
    shorter than its header says, with the offset within the record's own file; ``None`` if there is none."""
    bad = np.flatnonzero(status == 2)
    if len(bad) == 0:
        return None
    k = int(np.searchsorted(bounds, bad[0], side="right")) - 1
    return ValueError(f"miniSEED record at byte {int(table['offset'][bad[0]] - bases[k])}: payload holds fewer samples than "
                      "its header says")


def read_many(sources, device=0, dtype=None, device_resident=True):
    """``[read(s, device_resident=...) for s in sources]`` for miniSEED sources, with one ``vp_mseed_decode`` per sample
    kind for all of them: every file is scanned on the host, the bytes are concatenated, and one record table over the
    whole buffer is decoded at once.  Each returned ``Stream`` is what :func:`read_mseed` returns for that file -- the two
    build their traces with the same code, and a short payload is the same error -- and its traces are views into the
    decode buffers all files share."""
    bufs = [_as_bytes(s) for s in sources]
    r, seg, bounds, bases = many_tables(bufs)
    streams = [Stream() for _ in bufs]
    if len(r) == 0:
        return streams
    decoded = _decode(b"".join(bufs), r, bounds, bases, device, dtype, device_resident)
    first, last = _segment_ranges(seg)
    cut = np.searchsorted(first, bounds)  # a segment never reaches across a file boundary: file k owns [cut[k], cut[k + 1])
    for k, st in enumerate(streams):
        _add_traces(st, r, first[cut[k]:cut[k + 1]], last[cut[k]:cut[k + 1]], decoded, dtype, device_resident)
    return streams


def release_decode_scratch(device=0):
    """Free the device scratch `read_mseed` keeps per device between calls (vp_mseed_release_scratch); returns the bytes freed."""
    return release_scratch("vp_mseed_release_scratch", device)


# ----------------------------------------------------------------------------- traces to miniSEED
WRITE_RECLEN, WRITE_BYTEORDER, WRITE_QUALITY = 4096, ">", "D"  # ObsPy's defaults
WRITE_ENCODINGS = {"int32": (11, 10, 3, 1), "int16": (1,), "float32": (4,), "float64": (5,)}  # the first is the type's default
_WRITE_KINDS = {"int32": _lib.VP_SAMPLES_INT32, "int16": _lib.VP_SAMPLES_INT32, "float32": _lib.VP_SAMPLES_FLOAT32,
                "float64": _lib.VP_SAMPLES_FLOAT64}
_CODE_FIELDS = (("network", 2), ("station", 5), ("location", 2), ("channel", 3))


def rate_fields(rate):
    """The SEED sample-rate factor and multiplier the writer stores for ``rate`` (``vp_mseed_rate_fields``, host only): the
    smallest ``m`` in 1..32767 with ``rate * m`` an integer in 1..32767 gives ``(rate * m, 1 if m == 1 else -m)``; else an
    integer period ``1 / rate`` in 1..32767 gives ``(-1 / rate, 1)``.  ``ValueError`` where no pair gives ``rate`` back exactly."""
    f, m = C.c_int32(0), C.c_int32(0)
    if _lib.load().vp_mseed_rate_fields(float(rate), C.byref(f), C.byref(m)) < 0:
        raise ValueError(f"sampling rate {float(rate)!r} has no exact SEED factor / multiplier pair")
    return f.value, m.value


def _sample_type(tr):
    """The name of a trace's sample type without touching a device trace's host copy; masked traces are refused."""
    dev = device_backing(tr)
    if dev is not None:
        return str(dev.dtype).replace("torch.", "")
    if np.ma.isMaskedArray(tr.data):
        raise ValueError(f"{tr.id}: masked traces cannot be written; split the stream at its gaps first")
    return np.asarray(tr.data).dtype.name


def plan_write(stream_or_trace, reclen=None, encoding=None, byteorder=None, dataquality=None):
    """What :func:`write_mseed` will write, decided on the host before any GPU work: one dict per trace with samples, in
    stream order -- ``trace``, ``dtype`` (the sample type's name), ``kind`` (the library's sample kind), ``reclen``,
    ``encoding``, ``byteorder`` (``">"`` / ``"<"``), ``dataquality`` and the rate's ``factor`` / ``multiplier``.  Per trace a
    keyword wins over ``stats.mseed`` (what ``read`` recorded), which wins over ObsPy's defaults; every refusal of
    :func:`write_mseed` is raised here."""
    traces = [stream_or_trace] if isinstance(stream_or_trace, Trace) or not hasattr(stream_or_trace, "__iter__") else list(stream_or_trace)
    plan = []
    for tr in traces:
        if int(tr.stats.npts) == 0:
            continue
        dtype = _sample_type(tr)
        if dtype not in WRITE_ENCODINGS:
            raise ValueError(f"{tr.id}: samples of type {dtype} cannot be written (int32, int16, float32 and float64 can; "
                             "text records are not written)")
        was = tr.stats.get("mseed") or {}
        enc = encoding
        if enc is None:
            enc = was.get("encoding")
            if enc not in WRITE_ENCODINGS[dtype]:  # e.g. a Steim trace decoded or filtered to float32: the type decides
                enc = WRITE_ENCODINGS[dtype][0]
        elif enc not in WRITE_ENCODINGS[dtype]:
            raise ValueError(f"{tr.id}: encoding {enc!r} cannot hold {dtype} samples (allowed: "
                             f"{', '.join(str(e) for e in WRITE_ENCODINGS[dtype])})")
        rl = reclen
        if rl is None:
            rl = was.get("record_length")
            if not (isinstance(rl, int) and 128 <= rl <= 65536 and rl & (rl - 1) == 0):  # (a miniSEED 3 record has any length)
                rl = WRITE_RECLEN
        elif not (isinstance(rl, (int, np.integer)) and 128 <= rl <= 65536 and int(rl) & (int(rl) - 1) == 0):
            raise ValueError(f"reclen {rl!r} is not a power of two in 128..65536")
        if int(enc) == 11 and int(rl) == 65536:
            raise ValueError("reclen 65536 with encoding 11: a record could hold more samples than the header's 16-bit count")
        bo = byteorder if byteorder is not None else was.get("byteorder") or WRITE_BYTEORDER
        bo = {1: ">", 0: "<", ">": ">", "<": "<"}.get(bo)
        if bo is None:
            raise ValueError(f"byteorder {byteorder!r} is none of '>', '<', 1, 0")
        q = dataquality if dataquality is not None else was.get("dataquality") or WRITE_QUALITY
        if q not in ("D", "R", "Q", "M"):
            raise ValueError(f"dataquality {q!r} is none of D, R, Q, M")
        for field, width in _CODE_FIELDS:
            code = str(tr.stats[field])
            if len(code.encode("ascii", "replace")) > width:
                raise ValueError(f"{tr.id}: {field} {code!r} is longer than {width} characters")
        rate = float(tr.stats.sampling_rate)
        if not rate > 0:
            raise ValueError(f"{tr.id}: sampling rate {rate!r} is not positive")
        try:
            factor, mult = rate_fields(rate)
        except ValueError as e:
            raise ValueError(f"{tr.id}: {e}") from None
        plan.append(dict(trace=tr, dtype=dtype, kind=_WRITE_KINDS[dtype], reclen=int(rl), encoding=int(enc), byteorder=bo,
                         dataquality=q, factor=factor, multiplier=mult))
    return plan


def _encode_group(group, b1001, device):
    """One ``vp_mseed_encode`` for consecutive planned traces that share sample kind, encoding, record length and byte
    order: ``(bytes of the records, number of records)``.  Device traces are read where they lie -- the call gets the lowest
    address as its base and every trace's offset from it -- host traces are uploaded first."""
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", int(device))
    tensors = []
    for p in group:
        d = device_backing(p["trace"])
        if d is None:
            a = p["trace"].data  # (int16 travels as int32: upload_samples would make it float32)
            d = upload_samples(a.astype(np.int32) if p["dtype"] == "int16" else a, dev, "masked traces cannot be written")
        elif d.device != dev:
            d = d.to(dev)
        if d.dtype == torch.int16:
            d = d.to(torch.int32)
        tensors.append(d.contiguous())
    torch.cuda.current_stream(dev).synchronize()  # the library works on the null stream: the samples are complete first
    itemsize = tensors[0].element_size()
    base = min(t.data_ptr() for t in tensors)
    traces = (_lib.VpMseedTrace * len(group))()
    for k, (p, t) in enumerate(zip(group, tensors)):
        tr = p["trace"]
        assert (t.data_ptr() - base) % itemsize == 0
        traces[k].start_us, traces[k].sample_rate = UTCDateTime(tr.stats.starttime)._us, float(tr.stats.sampling_rate)
        traces[k].first_sample, traces[k].nsamples = (t.data_ptr() - base) // itemsize, int(t.shape[0])
        traces[k].quality = ord(p["dataquality"])
        for field, _ in _CODE_FIELDS:
            setattr(traces[k], field, str(tr.stats[field]).encode("ascii", "replace"))
    reclen, enc = group[0]["reclen"], group[0]["encoding"]
    # room for the worst case, one difference per word, so the call never has to be repeated
    per = 15 * (reclen // 64 - 1) - 2 if enc in (10, 11) else (reclen - 64) // {1: 2, 3: 4, 4: 4, 5: 8}[enc]
    cap = sum(-(-int(t.shape[0]) // per) for t in tensors) * reclen
    out = _host_buffer(cap)
    nbytes, nrec, bad_trace, bad_sample = C.c_size_t(0), C.c_int64(0), C.c_int64(-1), C.c_int64(-1)
    rc = lib.vp_mseed_encode(dev.index, C.c_void_p(base), _lib.VP_MEM_DEVICE, group[0]["kind"], traces, len(group), reclen, enc,
                             int(group[0]["byteorder"] == ">"), b1001, _lib.ptr(out), cap, C.byref(nbytes), C.byref(nrec),
                             C.byref(bad_trace), C.byref(bad_sample))
    if rc < 0 and bad_trace.value >= 0:
        why = ("does not fit int16 (encoding 1)" if enc == 1 else
               "differs from the sample before it by more than Steim-2's 30 bits hold (encoding 11)")
        raise ValueError(f"{group[bad_trace.value]['trace'].id}: sample {bad_sample.value} {why}; nothing was written")
    _lib.check(rc, "vp_mseed_encode")
    assert nbytes.value <= cap
    return out[:nbytes.value], int(nrec.value)


_HOST = threading.local()


def _host_buffer(nbytes):
    """The calling thread's output buffer of at least ``nbytes`` (grow-only; a write leaves a copy of what it used): pages
    that were touched once are not faulted in again by the next write."""
    buf = getattr(_HOST, "buf", None)
    if buf is None or len(buf) < nbytes:
        buf = _HOST.buf = np.empty(nbytes + nbytes // 4, np.uint8)
    return buf


def write_mseed(stream_or_trace, target=None, reclen=None, encoding=None, byteorder=None, dataquality=None,
                blockette1001=None, device=0):
    """A ``Stream`` or ``Trace`` as miniSEED 2 records, packed on the GPU (``vp_mseed_encode``): what the reference does with
    ``waveforms.write(path, format="MSEED")``.  ``target`` is a path or a binary file object; with ``None`` the call returns the
    ``bytes``, otherwise the number of records written.  Traces are written in stream order, empty ones are skipped, sequence
    numbers run from 1 through the file.

    Per trace a keyword wins over ``stats.mseed`` (``encoding``, ``byteorder``, ``record_length``, ``dataquality`` as ``read``
    recorded them), which wins over ObsPy's defaults: 4096-byte big-endian records of quality ``D``.  The default encoding
    follows the sample type: int32 -> 11 (Steim-2; 10, 3 and 1 on request), int16 -> 1, float32 -> 4, float64 -> 5.  A
    ``stats.mseed["encoding"]`` that no longer matches the sample type -- a Steim trace decoded or filtered to float32 -- gives
    way to the type's default; ObsPy refuses such a trace instead.  ``blockette1001``: ``None`` adds blockette 1001 to every
    record of a trace as soon as one of its records starts off the 100-microsecond grid, ``True`` / ``False`` force it.

    ``ValueError`` before any GPU work: other sample types and text records, an encoding the sample type cannot take
    (encoding 2 among them), masked traces, ``reclen`` not a power of two in 128..65536, a network / station / location /
    channel longer than 2 / 5 / 2 / 3 characters, a sampling rate that is not positive or has no exact SEED factor /
    multiplier pair (:func:`rate_fields`).  ``ValueError`` from the device, with nothing written to ``target``: a Steim-2
    difference beyond 30 bits or, under encoding 1, an int32 sample beyond int16 -- the message names the trace and its lowest
    such sample.  One deviation from a strict packer: a trace whose *first* sample does not fit 30 bits is written under
    Steim-2 with a first difference of 0 (decoders start from the record's X0 and never read it).

    A device-backed trace is read where it lies and its host copy is not materialised; a host trace is uploaded to
    ``cuda:device`` and takes the same kernels -- there is no host encoder.  All traces that share sample kind, encoding,
    record length and byte order go through one set of launches.  :func:`release_encode_scratch` frees the device scratch."""
    plan = plan_write(stream_or_trace, reclen, encoding, byteorder, dataquality)
    b1001 = -1 if blockette1001 is None else int(bool(blockette1001))
    parts, n_records, a = [], 0, 0
    while a < len(plan):
        b = a + 1
        while b < len(plan) and all(plan[b][k] == plan[a][k] for k in ("kind", "encoding", "reclen", "byteorder")):
            b += 1
        out, nrec = _encode_group(plan[a:b], b1001, device)
        if n_records:  # a later group: its sequence numbers go on where the group before stopped
            seq = (np.arange(nrec) + n_records + 1) % 1_000_000
            digits = (seq[:, None] // 10 ** np.arange(5, -1, -1)) % 10 + ord("0")
            out.reshape(nrec, plan[a]["reclen"])[:, :6] = digits.astype(np.uint8)
        parts.append(out.tobytes())  # (the buffer is the next group's too)
        n_records += nrec
        a = b
    data = b"".join(parts)
    if target is None:
        return data
    if hasattr(target, "write"):
        target.write(data)
    else:
        with open(os.fspath(target), "wb") as f:
            f.write(data)
    return n_records


def release_encode_scratch(device=0):
    """Free the device scratch `write_mseed` keeps per device between calls (vp_mseed_encode_release_scratch) and the calling
    thread's host buffer; returns the device bytes freed."""
    _HOST.buf = None
    return release_scratch("vp_mseed_encode_release_scratch", device)


def read_sac(source):
    """SAC binary (either byte order) -> Stream with one Trace.  Host only: the body is raw float32."""
    buf = _as_bytes(source)
    if len(buf) < 632:
        raise ValueError("not a SAC file: shorter than the 632-byte header")
    nv_le = struct.unpack_from("<i", buf, 76 * 4)[0]
    nv_be = struct.unpack_from(">i", buf, 76 * 4)[0]
    if 1 <= nv_le <= 7:
        bo = "<"
    elif 1 <= nv_be <= 7:
        bo = ">"
    else:
        raise ValueError("not a SAC file: header version field is neither byte order's 1..7")
    hf = np.frombuffer(buf, dtype=bo + "f4", count=70)
    hi = np.frombuffer(buf, dtype=bo + "i4", count=40, offset=280)
    ks = [buf[440 + 8 * i: 448 + 8 * i].decode("ascii", "replace").strip("\0 ") for i in range(24)]
    ks = ["" if k == "-12345" else k for k in ks]
    npts = int(hi[9])
    if npts < 0 or 632 + 4 * npts > len(buf):
        raise ValueError("SAC file is shorter than its header's npts")
    b = float(hf[5]) if hf[5] != -12345.0 else 0.0
    ref = datetime(int(hi[0]), 1, 1, tzinfo=timezone.utc) + timedelta(days=int(hi[1]) - 1, hours=int(hi[2]),
                                                                      minutes=int(hi[3]), seconds=int(hi[4]))
    d = ref - _EPOCH
    start_us = (d.days * 86400 + d.seconds) * 1_000_000 + int(hi[5]) * 1000 + int(round(b * 1e6))
    data = np.frombuffer(buf, dtype=bo + "f4", count=npts, offset=632).astype(np.float32)
    tr = Trace(data, dict(network=ks[21], station=ks[0], location=ks[3], channel=ks[20],
                          starttime=UTCDateTime._from_us(start_us), sampling_rate=float(np.float32(1.0) / hf[0])))
    tr.stats["_format"] = "SAC"
    return Stream([tr])


def read(source, format=None, device=0, dtype=None, device_resident=False):
    """``obspy.read`` for the two formats the reference's data pipeline handles (miniSEED, SAC);
    the format is auto-detected from the header unless given."""
    buf = _as_bytes(source)
    fmt = (format or ("MSEED" if _looks_like_mseed(buf) else "SAC")).upper()
    if fmt == "MSEED":
        return read_mseed(buf, device=device, dtype=dtype, device_resident=device_resident)
    if fmt == "SAC":
        return read_sac(buf)
    raise ValueError(f"unsupported waveform format {fmt!r} (MSEED and SAC are implemented)")


def stream_to_array(stream, component_order="ZNE"):
    """volpick/data/convert.py:26-70: (starttime, float64 array (len(component_order), samples) on
    the common time span with zero fill and row-wise demean, completeness)."""
    traces = list(stream)
    starttime = min(tr.stats.starttime for tr in traces)
    endtime = max(tr.stats.endtime for tr in traces)
    rate = float(traces[0].stats.sampling_rate)
    samples = int((endtime - starttime) * rate) + 1
    data = np.zeros((len(component_order), samples), dtype=np.float64)
    completeness = 0.0
    for ci, c in enumerate(component_order):
        sel = [tr for tr in traces if tr.stats.channel.endswith(c)]
        if len(sel) > 1:
            sel = sorted(sel, key=lambda tr: tr.stats.npts)
        cc = 0.0
        for tr in sel:
            s0 = int((tr.stats.starttime - starttime) * rate)
            n = min(len(tr.data), samples - s0)
            data[ci, s0:s0 + n] = tr.data[:n]
            cc += n
        completeness += min(1.0, cc / samples)
    data -= np.mean(data, axis=1, keepdims=True)
    return starttime, data, completeness / len(component_order)
