"""Many waveform files to picks in one pipelined call (``model.classify_files``).

``outs[k]`` is ``model.classify(volpick_amd.read(sources[k], device_resident=True), **kwargs)`` -- the same records in the
same order with the same bits -- but the host work of file k + 1 and its upload run beside file k's classification:

* ``workers`` host threads read the file, build its record table (``io.scan_segments``: one host-only library call), plan its
  station blocks from the headers (``io.plan_file_blocks``) and copy the bytes into the page-locked staging buffer of the
  file's ring slot.  They call nothing that touches a GPU or the model's handle.
* The calling thread owns the handle.  It sends the staged bytes up on a copy stream, makes the decode
  stream wait for that upload by an event, and launches ONE decode (``vp_mseed_decode_on``) that writes every station block
  of the file as float32, zero-filled and in component order -- no int32 intermediate, no torch kernel.  The blocks then take
  the routes of ``models._ClassifyRun`` exactly as ``classify()``'s do.
* A ring of ``depth + 1`` slots (staging bytes, device bytes, launch table) is grow-only and freed on return.  A slot is
  written again only behind the event of the decode that last read it.  No device-wide synchronisation anywhere.

A file without a fast route -- not miniSEED, a trace at another rate, a model with a filter, overlapping segments of one
component, text records in a used component, no records, or anything the scanner or the decoder refuses -- goes through
``read(..., device_resident=True)`` and ``classify``'s own assembly inside the same loop, and raises what that raises.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .io import _as_bytes, _looks_like_mseed, plan_file_blocks, read, scan_segments
from .stream import UTCDateTime, block_dict, warn_short_fragment

_I64P = C.POINTER(C.c_int64)
_GROW = 1.25  # a buffer that has to grow takes a quarter more than asked: file sizes of one archive scatter by less


def _pinned_bytes(n):
    """``stream.pinned_array(n, np.uint8)`` allocated page-locked from the start (``pinned_array`` page-locks a copy of a
    pageable array: 4 ms more for a station-day's bytes).  Freed, the pages go back to torch's host cache, so the ring of the
    next call costs no page-locking."""
    import torch

    return torch.empty(int(n), dtype=torch.uint8, pin_memory=True).numpy()


def _size_hint(source):
    """The source's size where it is known without reading it (bytes-like, a path), else 0."""
    try:
        return len(source) if isinstance(source, (bytes, bytearray, memoryview)) else os.path.getsize(os.fspath(source))
    except (TypeError, OSError):
        return 0


class _Slot:
    """One ring slot: the page-locked image of a file's bytes, the device copy, the decode's launch table (page-locked and
    device) and the event of the decode that last read them."""

    def __init__(self):
        self.staging = np.zeros(0, np.uint8)
        self.dev = self.table_host = self.table_dev = self.decode_done = None

    def grow_staging(self, nbytes):
        if nbytes > self.staging.size:
            self.staging = _pinned_bytes(int(nbytes * _GROW) + 4096)

    def grow_device(self, torch, dev, nbytes, n_recs):
        """Device bytes and launch table for a file of ``nbytes`` and ``n_recs`` records.  Called with the slot idle (its last
        decode waited for), so a buffer it replaces has no work pending."""
        if self.dev is None or nbytes + 4 > self.dev.numel():
            self.dev = torch.empty(int(nbytes * _GROW) + 4096, dtype=torch.uint8, device=dev)
        need = n_recs * _lib.VP_MSEED_TABLE_BYTES_PER_RECORD
        if self.table_dev is None or need > self.table_dev.numel():
            self.table_host = _pinned_bytes(int(need * _GROW) + 4096)
            self.table_dev = torch.empty(self.table_host.size, dtype=torch.uint8, device=dev)


class _Prepared:
    """What a worker hands back for one source: its bytes, and for a miniSEED file the scanner took, table and plan."""

    __slots__ = ("buf", "table", "plan", "staged", "ms")

    def __init__(self, buf):
        self.buf, self.table, self.plan, self.staged, self.ms = buf, None, None, False, {}


def _prepare(source, slot, plan_args):
    """Worker thread: host-only.  ``slot`` is this file's alone until the calling thread has finished the file."""
    t0 = time.perf_counter()
    p = _Prepared(_as_bytes(source))
    t1 = time.perf_counter()
    if _looks_like_mseed(p.buf):
        try:
            p.table, seg = scan_segments(p.buf)
        except _lib.VolpickHipError:
            return p  # read() raises it again, on the calling thread and with its own text
        p.plan = plan_file_blocks(p.table, seg, *plan_args, warn=False)
        t2 = time.perf_counter()
        if p.plan.reason is None and len(p.buf) <= slot.staging.size:
            slot.staging[:len(p.buf)] = np.frombuffer(p.buf, np.uint8)
            p.staged = True
        p.ms = dict(read_ms=(t1 - t0) * 1e3, scan_plan_ms=(t2 - t1) * 1e3, stage_ms=(time.perf_counter() - t2) * 1e3)
    return p


def decode_plan(torch, device, dev_bytes, nbytes, table, plan, table_host, table_dev, stream):
    """Enqueue on ``stream`` (a ``torch.cuda.Stream``, current while this runs) the one decode that writes every block of
    ``plan`` from the file image ``dev_bytes`` (uint8 tensor, ``nbytes`` of it) -> ``(rc, out, status)``: the library's return
    code, the file's float32 sample array and one status word per record of ``table``, both device tensors that are complete
    when ``stream`` gets there.  ``table_host`` (page-locked uint8 array) and ``table_dev`` (uint8 tensor) carry the launch
    table and must stay untouched until then."""
    lib = _lib.load()
    dev = torch.device("cuda", device)
    n_recs = len(table)
    table = np.ascontiguousarray(table)
    skip = plan.out_index < 0  # records of no block are decoded for their status alone
    out_index = np.where(skip, 0, plan.out_index).astype(np.int64)
    out_count = np.where(skip, 0, table["nsamples"]).astype(np.int64)
    n_decoded = C.c_int64(0)
    out = torch.empty(max(plan.n_out, 1), dtype=torch.float32, device=dev)
    status = torch.empty(n_recs, dtype=torch.int32, device=dev)
    rc = lib.vp_mseed_decode_on(
        device, C.c_void_p(dev_bytes.data_ptr()), nbytes, table.ctypes.data_as(C.POINTER(_lib.VpMseedRecord)),
        out_index.ctypes.data_as(_I64P), out_count.ctypes.data_as(_I64P), n_recs, _lib.VP_SAMPLES_FLOAT32,
        C.c_void_p(out.data_ptr()), plan.n_out, 1, C.c_void_p(status.data_ptr()), _lib.ptr(table_host),
        C.c_void_p(table_dev.data_ptr()), min(table_host.size, table_dev.numel()), C.byref(n_decoded),
        C.c_void_p(stream.cuda_stream))
    assert rc < 0 or n_decoded.value == n_recs  # scan_segments keeps no record without samples, and none is skipped here
    return rc, out, status


def plan_groups(plan, out):
    """The blocks of ``plan`` as ``models._group_stream``'s dicts, their data views into the decoded array ``out`` (a block
    no record feeds is host zeros, as the assembly makes it)."""
    groups = []
    for b in plan.blocks:
        c, n = b["shape"]
        data = out[b["offset"]:b["offset"] + c * n].view(c, n) if b["offset"] >= 0 else np.zeros((c, n), np.float32)
        groups.append(block_dict(data, b["network"], b["station"], b["location"], UTCDateTime._from_us(b["start_us"])))
    return groups


def pipeline_streams(model, torch, dev):
    """The copy stream and the decode stream of ``model``'s ``classify_files`` calls: made once per model and device, so that
    a process that makes many calls does not walk through torch's pool of streams."""
    made = model.__dict__.setdefault("_files_streams", {})
    if dev.index not in made:
        made[dev.index] = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    return made[dev.index]


def classify_files(model, sources, depth=2, workers=2, copy=True, _stats=None, **kwargs):
    """``[model.classify(read(s, device_resident=True), copy=copy, **kwargs) for s in sources]``, pipelined (module text).
    ``sources`` are what ``read`` takes: paths, bytes, file objects.  ``depth`` files ahead of the one being classified are
    read, planned and uploaded; ``workers`` threads do the host part.  Streams are not returned: a file's decoded samples
    are released when its picks are out.  ``_stats`` (a dict) collects the stage times of tools/files_timing.py."""
    from .models import _group_stream, _torch

    depth, workers = int(depth), int(workers)
    if depth < 1 or workers < 1:
        raise ValueError(f"depth and workers must be at least 1, got {depth} and {workers}")
    sources = list(sources)
    args = model._argdict(kwargs)
    specs = model._trigger_specs(args)
    if not sources:
        return []
    torch = _torch()
    model._ensure_handle()
    device = model._device_index
    dev = torch.device("cuda", device)
    stats = _stats if _stats is not None else {}

    def lap(key, t0):
        now = time.perf_counter()
        stats[key] = stats.get(key, 0.0) + (now - t0) * 1e3
        return now

    plan_args = (model.component_order, model.sampling_rate, model.in_samples, model._stream_filter() is not None)
    ring = [_Slot() for _ in range(depth + 1)]
    copy_stream, decode_stream = pipeline_streams(model, torch, dev)
    pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="volpick-files")
    futures, uploads, outs = {}, {}, []

    def submit(j):
        slot = ring[j % len(ring)]
        if slot.decode_done is not None:  # the file that had the slot: finished, and so is everything that read its buffers
            slot.decode_done.synchronize()
        slot.grow_staging(_size_hint(sources[j]))  # (a file object's size shows only when it is read: grown in upload())
        futures[j] = pool.submit(_prepare, sources[j], slot, plan_args)

    def upload(j, p):
        """File j's bytes -> its slot's device buffer, on the copy stream.  -> the event the decode waits for."""
        slot, n = ring[j % len(ring)], len(p.buf)
        if not p.staged:  # the staging buffer was too small when the worker looked: grown and filled here
            slot.grow_staging(n)
            slot.staging[:n] = np.frombuffer(p.buf, np.uint8)
        with torch.cuda.stream(copy_stream):  # (the slot's device buffers come from this stream's share of torch's allocator)
            slot.grow_device(torch, dev, n, len(p.table))
            if slot.decode_done is not None:
                copy_stream.wait_event(slot.decode_done)
            t = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)] if _stats is not None else None
            if t:
                t[0].record(copy_stream)
            slot.dev[:n].copy_(torch.from_numpy(slot.staging[:n]), non_blocking=True)
            done = torch.cuda.Event(enable_timing=t is not None)
            done.record(copy_stream)
        return done, (t[0] if t else None)

    def advance(j, block):
        """Move file j towards 'uploaded' as far as it goes without waiting (``block``: wait for its worker)."""
        if j >= len(sources) or j in uploads:
            return
        if j not in futures or not (block or futures[j].done()):
            return
        if not block and futures[j].exception() is not None:
            return  # raised when its turn comes, as the per-file loop would
        p = futures[j].result()
        uploads[j] = (p, upload(j, p) if p.plan is not None and p.plan.reason is None else None)

    def fallback(p):
        """The per-file call itself: whatever it computes, warns or raises is the contract."""
        stats["fallback_files"] = stats.get("fallback_files", 0) + 1
        st = read(p.buf, device=device, device_resident=True)
        return model._classify_groups(_group_stream(st, model.component_order, model.sampling_rate, copy, model.in_samples,
                                                    model._stream_filter()), args, specs)

    def fast(j, p, up):
        slot, plan = ring[j % len(ring)], p.plan
        t0 = time.perf_counter()
        with torch.cuda.stream(decode_stream):
            decode_stream.wait_event(up[0])
            rc, out, status = decode_plan(torch, device, slot.dev, len(p.buf), p.table, plan, slot.table_host, slot.table_dev,
                                          decode_stream)
            slot.decode_done = torch.cuda.Event()
            slot.decode_done.record(decode_stream)
            if rc == 0:
                status = status.cpu()  # waits for this file's upload and decode, and for nothing else
        if rc < 0:
            return fallback(p)  # a record the decoder refuses: read() says so in its own words
        if up[1] is not None:
            stats["upload_ms"] = stats.get("upload_ms", 0.0) + up[1].elapsed_time(up[0])
        t0 = lap("decode_wait_ms", t0)
        if (status == 2).any():
            return fallback(p)  # a payload shorter than its header says: read() raises for it
        for _ in range(plan.short_runs):
            warn_short_fragment()
        res = model._classify_groups(iter(plan_groups(plan, out)), args, specs)
        lap("classify_ms", t0)
        return res

    try:
        for j in range(min(depth + 1, len(sources))):
            submit(j)
        for k in range(len(sources)):
            t0 = time.perf_counter()
            advance(k, True)
            lap("wait_worker_ms", t0)
            for j in range(k + 1, k + depth + 1):
                advance(j, False)
            p, up = uploads.pop(k)
            del futures[k]
            for key, v in p.ms.items():
                stats[key] = stats.get(key, 0.0) + v
            outs.append(fast(k, p, up) if up is not None else fallback(p))
            del p, up
            if k + depth + 1 < len(sources):
                submit(k + depth + 1)  # the slot file k had
            for j in range(k + 1, k + depth + 1):
                advance(j, False)
        return outs
    finally:
        for f in futures.values():
            f.cancel()
        pool.shutdown(wait=True)
        for ev in [s.decode_done for s in ring if s.decode_done is not None]:
            ev.synchronize()  # nothing of this call is in flight when its buffers go
        copy_stream.synchronize()
