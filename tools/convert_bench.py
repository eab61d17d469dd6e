"""Event miniSEED files -> a device-resident waveform bank: the route of volpick_amd/convert.py (`bank_from_mseed`: one decode
launch per sample kind, one `vp_bank_assemble`) against the route available before it (per file `read(device_resident=True)`,
`detrend("demean")` on the device, host `io.stream_to_array`, then `WaveformBank(list, onsets)`), and the assembly launches
alone against their traffic floor.

Files: `--files` copies of one event -- three components, four 4096-byte Steim-2 records each (about 120 s at 100 Hz), cut
from the committed fixture tests/golden/bench_steim2_6min.mseed.  The two routes take turns, `--repeats` times each after one
untimed turn, on a host clock around work that ends in a device synchronise; medians are reported.  The assembly alone:
device events around `vp_bank_assemble` into a fresh bank (created outside the timed region), on the files' own decoded
traces and on `--events` synthetic events of 3 x 12,000 int32 samples, whose sources and bank together exceed the Infinity
Cache.  The events bracket the whole call, so they include the host's checking and table building, during which the device
idles; `--assemble-only` under `rocprofv3 --kernel-trace --stats` gives the three kernels' own times.  Floor: (2 x source bytes + bank bytes) / 6.29 TB/s, the measured copy rate of MI355X_MICROARCH / BASELINE.md.

    python tools/convert_bench.py [--files 256] [--events 4096] [--repeats 7] [--out profiles/convert_bench.txt]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

COPY_RATE = 6.29e12  # bytes / s


def event_file():
    """One event's bytes: the first four records of each channel of the fixture."""
    import volpick_amd.io as vio

    blob = (ROOT / "tests" / "golden" / "bench_steim2_6min.mseed").read_bytes()
    recs = vio.scan_mseed(blob)
    parts = []
    for ch in np.unique(recs["channel"]):
        mine = recs[recs["channel"] == ch]
        mine = mine[np.argsort(mine["start_us"])][:4]
        parts += [blob[int(r["offset"]):int(r["offset"]) + int(r["reclen"])] for r in mine]
    return b"".join(parts)


def new_route(files, meta):
    import torch
    from volpick_amd import bank_from_mseed

    bank, table = bank_from_mseed(files, meta)
    torch.cuda.synchronize()
    return bank


def old_route(files, meta):
    import torch
    import volpick_amd.io as vio
    from volpick_amd.generate import WaveformBank

    arrays, p, s = [], [], []
    for f, pt, st_ in zip(files, meta["trace_p_arrival_time"], meta["trace_s_arrival_time"]):
        st = vio.read(f, device_resident=True).detrend("demean")
        start, data, _ = vio.stream_to_array(st)
        arrays.append(data)
        p.append(int((vio.UTCDateTime(pt) - start) * 100))
        s.append(int((vio.UTCDateTime(st_) - start) * 100))
    bank = WaveformBank(arrays, {"P": np.array(p, float), "S": np.array(s, float)})
    torch.cuda.synchronize()
    return bank


def time_assemble(pieces, lengths, iters):
    """Median ms of `vp_bank_assemble` (device events) into a fresh bank, and its traffic in bytes."""
    import torch
    from volpick_amd import _lib

    lib = _lib.load()
    lengths = np.ascontiguousarray(lengths, np.int64)
    onsets = np.full((len(lengths), 4), np.nan)
    stream = torch.cuda.current_stream()
    size = {_lib.VP_SAMPLES_INT32: 4, _lib.VP_SAMPLES_FLOAT32: 4, _lib.VP_SAMPLES_FLOAT64: 8}
    traffic = int(2 * sum(int(n) * size[int(k)] for n, k in zip(pieces["mean_n"], pieces["kind"])) + 12 * lengths.sum())
    ms = []
    for it in range(iters + 2):
        h = C.c_void_p()
        _lib.check(lib.vp_bank_create(0, len(lengths), int(3 * lengths.sum()), C.byref(h)), "vp_bank_create")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        _lib.check(lib.vp_bank_assemble(h, 0, len(lengths), pieces.ctypes.data_as(C.c_void_p), len(pieces),
                                        lengths.ctypes.data_as(C.POINTER(C.c_int64)), onsets.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.c_void_p(stream.cuda_stream)), "vp_bank_assemble")
        e1.record(stream)
        e1.synchronize()
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
        _lib.check(lib.vp_bank_destroy(h), "vp_bank_destroy")
    return statistics.median(ms), traffic


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--assemble-only", action="store_true",
                    help="skip the two routes: the assembly calls alone, e.g. under `rocprofv3 --kernel-trace --stats` for the "
                         "time of assemble_stats_kernel / assemble_means_kernel / assemble_write_kernel themselves")
    args = ap.parse_args()

    import torch
    import volpick_amd.io as vio
    from volpick_amd import _lib
    from volpick_amd.convert import piece_table, plan_event
    from volpick_amd.generate import ASSEMBLE_PIECE

    assert torch.cuda.is_available(), "convert_bench.py measures on the GPU; there is no CPU fallback"
    one = event_file()
    files = [one] * args.files
    t0 = vio.read(one, device_resident=True)[0].stats.starttime
    meta = {"trace_p_arrival_time": [str(t0 + 40.0)] * args.files, "trace_s_arrival_time": [str(t0 + 52.5)] * args.files}

    # the two routes give the same bank
    a, b = new_route(files[:3], {k: v[:3] for k, v in meta.items()}), old_route(files[:3], {k: v[:3] for k, v in meta.items()})
    worst = max(float(np.abs(a.trace(i) - b.trace(i)).max()) for i in range(3))
    same_onsets = bool(np.array_equal(a.onsets, b.onsets, equal_nan=True))
    npts = int(a.lengths[0])
    a.close(), b.close()

    times = {"new": [], "old": []}
    for rep in range(0 if args.assemble_only else args.repeats + 1):
        for name, fn in (("new", new_route), ("old", old_route)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            bank = fn(files, meta)
            dt = time.perf_counter() - t
            bank.close()
            if rep:
                times[name].append(dt * 1e3)
    new_ms, old_ms = (statistics.median(times[k]) if times[k] else float("nan") for k in ("new", "old"))

    # the assembly alone, on the files' decoded traces ...
    streams = vio.read_many(files)
    plans = [plan_event(st, p, s) for st, p, s in zip(streams, meta["trace_p_arrival_time"], meta["trace_s_arrival_time"])]
    pieces, keep = piece_table(plans)
    asm_ms, asm_bytes = time_assemble(pieces, [pl["samples"] for pl in plans], 20)
    # ... and on synthetic events past the Infinity Cache
    n, L = args.events, 12000
    src = torch.randint(-30000, 30000, (n * 3, L), dtype=torch.int32, device="cuda")
    big = np.zeros(3 * n, ASSEMBLE_PIECE)
    big["src"] = src.data_ptr() + np.arange(3 * n, dtype=np.uint64) * np.uint64(4 * L)
    big["mean_n"] = big["keep_n"] = L
    big["trace"], big["component"] = np.arange(3 * n) // 3, np.arange(3 * n) % 3
    big["kind"] = _lib.VP_SAMPLES_INT32
    big_ms, big_bytes = time_assemble(big, np.full(n, L), 10)

    result = {
        "files": args.files, "samples_per_event": npts, "repeats": args.repeats,
        "bank_from_mseed_ms": round(new_ms, 3), "parent_route_ms": round(old_ms, 3), "ratio_old_over_new": round(old_ms / new_ms, 2),
        "bank_from_mseed_ms_all": [round(v, 2) for v in times["new"]], "parent_route_ms_all": [round(v, 2) for v in times["old"]],
        "routes_max_abs_diff": worst, "routes_same_onsets": same_onsets,
        "assemble_files_ms": round(asm_ms, 4), "assemble_files_bytes": asm_bytes,
        "assemble_files_floor_fraction": round(asm_bytes / COPY_RATE * 1e3 / asm_ms, 4),
        "assemble_events": n, "assemble_events_ms": round(big_ms, 4), "assemble_events_bytes": big_bytes,
        "assemble_events_floor_ms": round(big_bytes / COPY_RATE * 1e3, 4),
        "assemble_events_floor_fraction": round(big_bytes / COPY_RATE * 1e3 / big_ms, 4),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
