#!/usr/bin/env python3
"""Many miniSEED station-days to picks: the per-file loop, read_many + one classify, and classify_files, in one process.

  python tools/files_timing.py [--out profiles/files_pipeline_timing.txt] [--hours 24] [--reps 5]

Inputs: synthetic Steim-2 station-days (three components, 100 Hz), 32 for PhaseNet and 8 for EQTransformer (the counts
README.md uses for many station-days), once with 4096-byte and once with 512-byte records.  The 4096-byte day is the
committed six-minute fixture tests/golden/bench_steim2_6min.mseed tiled by patching start times (bench.py's
station_day_mseed); the 512-byte day is the fixture's samples written again by the oracle's encoder and tiled the same way.
Every file is its own station (the station code of its records is patched) and its own host copy, so that a pass over the
files reads each from memory, not from a cache, and the device buffers rotate with them.

Legs, per model and record length, all timed as wall time around the calls with the device idle before and after:
  (i)   the per-file loop   [model.classify(read(b, device_resident=True), **kw) for b in files], --reps times: its spread;
  (ii)  read_many(files), the streams joined, ONE classify;
  (iii) model.classify_files(files, depth, workers) for depth 1-3 and workers 1, 2, 4 (median of 3), and for the best of
        them the stage split (worker: read, scan + plan, copy to page-locked memory; calling thread: waiting for a worker,
        upload (HIP events), decode + wait, classify + emit);
  (iv)  classify of the same files already decoded on the device: the device-resident rate, for scale.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "files_pipeline_timing.txt"))
ap.add_argument("--hours", type=int, default=24)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--files", type=int, nargs=2, default=(32, 8), help="station-days for PhaseNet and for EQTransformer")
opt = ap.parse_args()

import torch  # noqa: E402

import volpick_amd as va  # noqa: E402
import volpick_amd.io as vio  # noqa: E402
from oracle import mseed as OM  # noqa: E402
from volpick_amd import _lib  # noqa: E402

lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def tiled(blob0, tiles):
    """`blob0` (miniSEED 2 records of some minutes) `tiles` times in a row, start times moved on by its span."""
    import struct
    from datetime import datetime, timedelta, timezone

    recs = vio.scan_mseed(blob0)
    span = int(round(int(recs["nsamples"][recs["channel"] == recs["channel"][0]].sum()) * 1e6 / float(recs["sample_rate"][0])))
    epoch, parts = datetime(1970, 1, 1, tzinfo=timezone.utc), []
    for k in range(tiles):
        b = bytearray(blob0)
        for r in recs:
            t = epoch + timedelta(microseconds=int(r["start_us"]) + k * span)
            struct.pack_into(">HHBBBBH", b, int(r["offset"]) + 20, t.year, t.timetuple().tm_yday, t.hour, t.minute, t.second, 0,
                             t.microsecond // 100)
        parts.append(bytes(b))
    return b"".join(parts)


def stations(day, reclen, n):
    """`n` copies of the file `day`, file k's records carrying station code S000k."""
    a = np.frombuffer(day, np.uint8).reshape(-1, reclen)
    out = []
    for k in range(n):
        b = a.copy()
        b[:, 8:13] = np.frombuffer(f"S{k:04d}".encode(), np.uint8)
        out.append(b.tobytes())
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def n_picks(outs):
    return sum(len(o.picks) for o in outs)


def run(model, name, kw, files, reclen):
    lib = _lib.load()
    n_files = len(files)
    n_samples = int(vio.scan_mseed(files[0])["nsamples"].sum()) // 3
    windows = int(lib.vp_window_starts(n_samples, model.in_samples, model._argdict(dict(kw))["overlap"], None, 0))
    rate = lambda ms: windows / ms * 1e3  # noqa: E731
    say(f"--- {name}, {n_files} station-days of {len(files[0]) / 1e6:.1f} MB in {reclen}-byte records, {n_samples} samples x 3, "
        f"{windows} windows each; {kw}")
    per_file = lambda: [model.classify(va.read(b, device_resident=True), **kw) for b in files]  # noqa: E731
    want = n_picks(per_file())  # warm-up: contexts, scratch
    loop = sorted(wall(per_file)[0] / n_files for _ in range(opt.reps))
    spread = loop[-1] - loop[0]
    say(f"(i)   per-file loop, {opt.reps} passes: {' '.join(f'{v:.3f}' for v in loop)} ms per file; median "
        f"{statistics.median(loop):.3f}, spread {spread:.3f}; {rate(statistics.median(loop)):,.0f} windows/s; {want} picks")

    def many():
        st = va.Stream()
        for s in va.read_many(files):
            st += s
        return [model.classify(st, **kw)]

    assert n_picks(many()) == want
    t_many = statistics.median(wall(many)[0] / n_files for _ in range(3))
    say(f"(ii)  read_many + one classify: {t_many:.3f} ms per file; {rate(t_many):,.0f} windows/s")

    best = None
    for depth in (1, 2, 3):
        for workers in (1, 2, 4):
            call = lambda: model.classify_files(files, depth=depth, workers=workers, **kw)  # noqa: E731
            assert n_picks(call()) == want
            t = statistics.median(wall(call)[0] / n_files for _ in range(3))
            say(f"(iii) classify_files depth {depth} workers {workers}: {t:.3f} ms per file; {rate(t):,.0f} windows/s")
            if best is None or t < best[0]:
                best = (t, depth, workers)
    stats = {}
    model.classify_files(files, depth=best[1], workers=best[2], _stats=stats, **kw)
    per = {k: v / n_files for k, v in stats.items() if k.endswith("_ms")}
    say(f"      best: depth {best[1]} workers {best[2]}, {best[0]:.3f} ms per file; stage split per file (ms) -- worker threads: "
        f"read {per.get('read_ms', 0):.3f}, scan + plan {per.get('scan_plan_ms', 0):.3f}, copy to page-locked "
        f"{per.get('stage_ms', 0):.3f}; calling thread: waiting for a worker {per.get('wait_worker_ms', 0):.3f}, upload (device "
        f"time) {per.get('upload_ms', 0):.3f}, decode + wait {per.get('decode_wait_ms', 0):.3f}, classify + emit "
        f"{per.get('classify_ms', 0):.3f}; files left to read(): {stats.get('fallback_files', 0)}")

    streams = [va.read(b, device_resident=True) for b in files]
    resident = lambda: [model.classify(s, **kw) for s in streams]  # noqa: E731
    assert n_picks(resident()) == want
    t_res = statistics.median(wall(resident)[0] / n_files for _ in range(3))
    say(f"(iv)  classify of device-resident streams: {t_res:.3f} ms per file; {rate(t_res):,.0f} windows/s")
    gain = statistics.median(loop) - best[0]
    say(f"      best (iii) is {gain:.3f} ms per file below (i)'s median ({statistics.median(loop) / best[0]:.2f}x) and "
        f"{loop[0] - best[0]:.3f} below its fastest pass, (i)'s spread is {spread:.3f}: "
        f"{'beats the loop' if loop[0] - best[0] > spread else 'does NOT beat the loop by more than its spread'}; "
        f"(iii) / (iv) rate = {t_res / best[0]:.2f}")
    say()
    del streams


def main():
    say(f"files to picks, {time.strftime('%Y-%m-%d')}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say()
    fixture = (ROOT / "tests" / "golden" / "bench_steim2_6min.mseed").read_bytes()
    samples = np.load(ROOT / "tests" / "golden" / "bench_steim2_6min_samples.npz")
    recs = vio.scan_mseed(fixture)
    t0 = int(recs["start_us"].min())
    small = OM.write_mseed([dict(network="XX", station="S0000", location="", channel=c, start_us=t0, rate=100.0, data=samples[c])
                            for c in ("HHZ", "HHN", "HHE")], reclen=512)
    days = {4096: tiled(fixture, opt.hours * 10), 512: tiled(small, opt.hours * 10)}
    models = [(va.PhaseNet, "PhaseNet", dict(batch_size=256, overlap=1500, blinding=(0, 0), stacking="avg"), opt.files[0]),
              (va.EQTransformer, "EQTransformer", dict(batch_size=256, overlap=5500, blinding=(500, 500), stacking="avg",
                                                       P_threshold=0.2, S_threshold=0.2), opt.files[1])]
    for cls, name, kw, n in models:
        model = cls.from_pretrained("volpick").cuda()
        for reclen, day in days.items():
            run(model, name, kw, stations(day, reclen, n), reclen)
        model._release()
    Path(opt.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
