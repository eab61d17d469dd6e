#!/usr/bin/env python3
"""Record tests/golden/classify_call_trace.json: the SEQUENCE of library calls behind classify() / annotate() / classify_files(),
and their picks.

The order in which the picker's host path issues uploads, submits and collects over the device contexts is what overlaps one
block's copy with another's compute; no result depends on it, so no result test notices when it moves.  This fixture pins it
across a change of volpick_amd/models.py that must leave it alone: check out the commit whose behaviour is the reference,
build it, run this script on the GPU (twice: the two files must be identical), commit the file, then change the host path.
tests/test_gpu_classify_calls.py runs the same cases and compares for equality.

    python tools/record_classify_call_trace.py [OUT.json]      (default: tests/golden/classify_call_trace.json)

`CallRecorder` stands where the loaded library stands (`volpick_amd._lib._lib`, what `_lib.load()` returns) for the duration
of one call, notes one row per `vp_annotate`, `vp_classify_submit`, `vp_classify_collect`, `vp_classify_multi` and
`vp_pick_rows`, and forwards every call unchanged.  Only outputs are stored; the inputs are the seeded streams of `CASES`.
"""
import ctypes as C
import json
import sys
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden" / "classify_call_trace.json"
# one row per recorded call; -1 where the call has no such argument.  `samples`: the block's sample count (multi: the list of
# block lengths); `cap`: the result capacity (multi: [per row, total])
COLUMNS = ["function", "context", "slot", "samples", "n_specs", "cap", "overlap", "blind_left", "blind_right", "stacking", "batch"]
MAX_BATCH = 8  # makes "long" cheap (tests/test_gpu_async.py): from 48 windows for PhaseNet, 64 for EQTransformer


class CallRecorder:
    """Forwards to ``lib``; ``rows`` receives one COLUMNS row per recorded call, written after the call has returned (the
    context index is the handle's position in ``[_handle] + _extra_handles``, and a context is created on first use)."""

    def __init__(self, lib, model):
        self._lib, self._model, self.rows = lib, model, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        row = getattr(self, "_row_" + name, None)
        if row is None:
            return fn

        def call(*a):
            rc = fn(*a)
            self.rows.append([name[3:], self._context(a[0])] + row(a))
            return rc

        return call

    def _context(self, h):
        handles = [self._model._handle] + list(self._model._extra_handles)
        return [x.value for x in handles].index(h.value)

    @staticmethod
    def _five(a, i):
        return [int(v) for v in a[i:i + 5]]

    def _row_vp_annotate(self, a):  # (h, x, mem, n, overlap, bl, br, stacking, batch, out, mem, fv, lv, nw)
        return [-1, int(a[3]), -1, -1] + self._five(a, 4)

    def _row_vp_classify_submit(self, a):  # (h, slot, x, mem, n, <five>, specs, n_specs, out, mem, cap)
        return [int(a[1]), int(a[4]), int(a[11]), int(a[14])] + self._five(a, 5)

    def _row_vp_classify_collect(self, a):  # (h, slot, fv, lv, nw, on, off, peak, value, spec_of, cap, found)
        return [int(a[1]), -1, -1, int(a[10])] + [-1] * 5

    def _row_vp_classify_multi(self, a):  # (h, flat, mem, offsets, lens, K, <five>, specs, n_specs, ..., cap_per_row, cap, found)
        lens = C.cast(a[4], C.POINTER(C.c_int64))
        return [-1, [int(lens[i]) for i in range(int(a[5]))], int(a[12]), [int(a[24]), int(a[25])]] + self._five(a, 6)

    def _row_vp_pick_rows(self, a):  # (h, rows, n, specs, n_specs, on, off, peak, value, spec_of, cap, found)
        return [-1, int(a[2]), int(a[4]), int(a[10])] + [-1] * 5


# ------------------------------------------------------------------------------------------------------------ the cases
def _station(name, n, seed, k, counts=False, device=False):
    """Three traces of one station: seeded synthetic samples, float32 rows, int32 counts or device arrays."""
    import torch

    from volpick_amd import Trace, UTCDateTime
    from volpick_amd.synthetic import synthetic_stream_array

    data = synthetic_stream_array(n, seed=seed, n_events=max(2, n // 50_000))[0]
    t0 = UTCDateTime("2023-03-03T03:03:03") + 10 * k
    out = []
    for i, c in enumerate("ZNE"):
        hdr = dict(network="XX", station=name, location="", channel="HH" + c, starttime=t0, sampling_rate=100.0)
        if device:
            out.append(Trace(header=hdr, device_data=torch.from_numpy(data[i]).cuda()))
        else:
            out.append(Trace((data[i] * 1000).astype(np.int32) if counts else data[i], hdr))
    return out


def _stream(stations):
    from volpick_amd import Stream

    return Stream([tr for k, (name, n, kind) in enumerate(stations)
                   for tr in _station(name, n, 900 + k, k, counts=kind == "counts", device=kind == "device")])


def _model(cls_name):
    import volpick_amd as va

    m = getattr(va, cls_name).from_pretrained("volpick")
    m._max_batch = MAX_BATCH
    return m.cuda()


PN_T, PN_LONG = 3001, 3001 + (3001 - 1500) * 90 + 5      # 138,096 samples: 92 windows >= 2 * 8 * 3
EQT_LONG = 33 * 6000 + 5                                 # 198,005 samples: 65 windows at overlap 3000 >= 2 * 8 * 4, and >= 8 segments' worth
PN_KW = dict(overlap=1500, P_threshold=0.25, S_threshold=0.25)
# Stations sort by name, so this is the order classify() meets them in.  A*: three long host blocks in a row, the second as
# int32 counts (both sets of submit slots, one segment per context for the block behind, the first block's finer cut); B*: five
# short host blocks, more than the three contexts (the oldest is collected to make room; the long jobs are finished before the
# first); C0: a long block behind pending short ones; D*: four short device-resident blocks of 13, 15, 9 and 11 windows under
# a budget of 40 per call: one multi call of three blocks, then a chunk of exactly one block (the single-submit path)
FULL = [("A0", PN_LONG, "host"), ("A1", PN_LONG + 777, "counts"), ("A2", PN_LONG, "host"),
        ("B0", 20_000, "host"), ("B1", 3 * PN_T, "host"), ("B2", 14_000, "host"), ("B3", 17_001, "host"), ("B4", 11_111, "host"),
        ("C0", PN_LONG + 1234, "host"),
        ("D0", 20_000, "device"), ("D1", 23_000, "device"), ("D2", 15_000, "device"), ("D3", 18_000, "device")]
SMALL = [("A0", PN_LONG, "host"), ("A1", PN_LONG + 777, "counts"), ("B0", 20_000, "host"), ("B1", 3 * PN_T, "host"),
         ("C0", PN_LONG, "host"), ("D0", 20_000, "device"), ("D1", 15_000, "device")]
WINDOW_BUDGET = 40


def _records(out):
    bits = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    return {"picks": [[p.trace_id, p.phase, p.start_time._us, p.end_time._us, p.peak_time._us, bits(p.peak_value)] for p in out.picks],
            "detections": [[d.trace_id, d.start_time._us, d.end_time._us, bits(d.peak_value)] for d in out.detections]}


def case_phasenet_classify(record):
    m, st = _model("PhaseNet"), _stream(FULL)
    m._max_windows_per_call = WINDOW_BUDGET
    return _records(record(m, lambda: m.classify(st, **PN_KW)))


def case_phasenet_classify_profiled(record):
    """Profiled mode: every upload of a long block, then every submit, and each long block finished before the next."""
    m, st = _model("PhaseNet"), _stream(SMALL)
    m._max_windows_per_call = WINDOW_BUDGET
    m._timing = {}
    out = _records(record(m, lambda: m.classify(st, **PN_KW)))
    out["timing_keys"] = sorted(m._timing)
    return out


def case_phasenet_annotate(record):
    m, st = _model("PhaseNet"), _stream([("A0", PN_LONG, "host"), ("B0", 20_000, "host")])
    traces = record(m, lambda: m.annotate(st, overlap=1500))
    return {"traces": [[tr.id, tr.stats.starttime._us, int(tr.stats.npts), zlib.crc32(np.ascontiguousarray(tr.data).tobytes())]
                       for tr in traces]}


def case_eqtransformer_classify(record):
    m, st = _model("EQTransformer"), _stream([("A0", EQT_LONG, "host"), ("A1", EQT_LONG + 333, "counts"), ("B0", 14_000, "host")])
    return _records(record(m, lambda: m.classify(st, overlap=3000, P_threshold=0.2, S_threshold=0.2)))


def _file(stations, extra=()):
    """The stations' traces as int32 counts (seeded as ``_stream``'s) plus the trace dicts ``extra``: one miniSEED 2 file."""
    from oracle import mseed as OM

    traces = [dict(network=tr.stats.network, station=tr.stats.station, location=tr.stats.location, channel=tr.stats.channel,
                   start_us=tr.stats.starttime._us, rate=tr.stats.sampling_rate, data=tr.data)
              for k, (name, n, seed) in enumerate(stations) for tr in _station(name, n, seed, k, counts=True)]
    return OM.write_mseed(traces + list(extra), reclen=4096, encoding=OM.ENC_INT32)


def case_phasenet_classify_files(record):
    """classify_files() goes through classify()'s loop, whichever way a file takes: F0 is one long block; G0, G1 are planned
    from the headers and share one multi call; the third file has the same two stations and a 50 Hz trace, so it has no plan
    and is read and assembled as classify() does (that trace, resampled, is a third block of the multi call)."""
    m = _model("PhaseNet")
    m._max_windows_per_call = WINDOW_BUDGET
    slow = _station("H2", 4000, 925, 2, counts=True)[0]
    slow = dict(network="XX", station="H2", location="", channel="HHZ", start_us=slow.stats.starttime._us, rate=50.0, data=slow.data)
    files = [_file([("F0", PN_LONG, 910)]), _file([("G0", 20_000, 920), ("G1", 15_000, 921)]),
             _file([("H0", 20_000, 922), ("H1", 15_000, 923)], [slow])]
    outs = [_records(out) for out in record(m, lambda: m.classify_files(files, depth=2, workers=1, **PN_KW))]
    return {key: [[k] + row for k, out in enumerate(outs) for row in out[key]] for key in ("picks", "detections")}


CASES = {"phasenet_classify": case_phasenet_classify, "phasenet_classify_profiled": case_phasenet_classify_profiled,
         "phasenet_annotate": case_phasenet_annotate, "eqtransformer_classify": case_eqtransformer_classify,
         "phasenet_classify_files": case_phasenet_classify_files}


def run_case(name, install):
    """One case -> {"calls": rows, ...results}.  ``install(recorder_or_None)`` puts the recorder where the loaded library is
    (None: the library back); the test passes pytest's monkeypatch, ``main`` sets the module global."""
    from volpick_amd import _lib

    calls = []

    def record(model, fn):
        rec = CallRecorder(_lib.load(), model)
        install(rec)
        try:
            return fn()
        finally:
            install(None)
            calls.extend(rec.rows)

    out = CASES[name](record)
    return dict(calls=calls, **out)


def dumps(result):
    """JSON with one call / pick row per line."""
    lines = ["{", f' "columns": {json.dumps(COLUMNS)},']
    for ci, (name, case) in enumerate(result["cases"].items()):
        lines.append(f' {json.dumps(name)}: {{')
        for ki, (key, rows) in enumerate(case.items()):
            end = "," if ki + 1 < len(case) else ""
            if key == "timing_keys":
                lines.append(f'  {json.dumps(key)}: {json.dumps(rows)}{end}')
                continue
            lines.append(f'  {json.dumps(key)}: [')
            lines += [f'   {json.dumps(r, separators=(",", ":"))}{"," if i + 1 < len(rows) else ""}' for i, r in enumerate(rows)]
            lines.append(f'  ]{end}')
        lines.append(" }" + ("," if ci + 1 < len(result["cases"]) else ""))
    return "\n".join(lines + ["}"]) + "\n"


def load_golden(path=GOLDEN):
    doc = json.loads(Path(path).read_text())
    return {k: v for k, v in doc.items() if k != "columns"}


def main():
    from volpick_amd import _lib

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    lib = _lib.load()

    def install(rec):
        _lib._lib = rec if rec is not None else lib

    result = {"cases": {name: run_case(name, install) for name in CASES}}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(dumps(result))
    print(out, {name: {k: len(v) for k, v in case.items()} for name, case in result["cases"].items()}, "bytes:", out.stat().st_size)


if __name__ == "__main__":
    main()
