"""Frequency index and SNR on the device (vp_bank_attributes / vp_attributes) next to the float64 host restatement
(tests/attributes_f64.py: scipy.fft and np.percentile per row in a Python loop, one thread) on the same rows and the same
machine.

    python tools/bench_attributes.py [--traces 2000] [--length 6000] [--hours 24] [--repeats 3] [--out profiles/attributes.json]

1. ``bank_attributes`` of a synthetic bank of --traces traces of --length samples (P and S onsets in every trace): wall time of
the whole call (host planning, row upload, three kernels, result download), the planning alone, and the host restatement of
the same traces.  2. ``pick_attributes`` for the picks PhaseNet finds in one synthetic station-day of --hours hours,
device-resident: wall time of the whole call (block assembly, planning, one launch), and the host restatement on a window cut
around every pick (the dead-channel sum over the whole day, which the restatement would repeat per pick, is left out of the
host's time).  The worst |device - host| over the trace frequency index and the mean SNR is reported with the timings.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE))


def _timed(fn, repeats):
    fn()  # untimed: scratch, module load
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, min(ts), float(np.median(ts))


def _worst(got, want):
    d = np.abs(np.asarray(got) - np.asarray(want))
    return float(np.nanmax(d)) if np.isfinite(d).any() else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=2000)
    ap.add_argument("--length", type=int, default=6000)
    ap.add_argument("--hours", type=float, default=24.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement's timing (and the difference with it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import volpick_amd as va
    from tests import attributes_f64 as A
    from volpick_amd import attributes as VA
    from volpick_amd.generate import WaveformBank
    from volpick_amd.synthetic import synthetic_stream_array

    torch.set_num_threads(1)
    result = {"device": torch.cuda.get_device_name(0)}

    # ---- 1. a bank
    rng = np.random.default_rng(0)
    waves = np.stack([synthetic_stream_array(a.length, 1000 + i, n_events=0)[0] for i in range(min(a.traces, 64))])
    waves = waves[rng.integers(0, len(waves), a.traces)] * rng.uniform(0.5, 2.0, (a.traces, 1, 1)).astype(np.float32)
    p = rng.integers(a.length // 3, a.length // 2, a.traces)
    s = p + rng.integers(300, 900, a.traces)
    t = np.arange(1500) / 100.0
    for i in range(a.traces):  # an 8 Hz P and a 4 Hz S burst, as synthetic_stream_array's events
        for at, hz, amp in ((p[i], 8.0, 1.0), (s[i], 4.0, 1.5)):
            n = min(1500, a.length - at)
            waves[i, :, at : at + n] += (amp * np.exp(-t[:n] / 1.5) * np.sin(2 * np.pi * hz * t[:n])).astype(np.float32)
    bank = WaveformBank(waves, {"P": p.astype(np.float64), "S": s.astype(np.float64)})
    cols, best, med = _timed(lambda: VA.bank_attributes(bank), a.repeats)
    _, plan_best, _ = _timed(lambda: VA.plan_rows(bank.lengths, bank.onsets[:, 0], bank.onsets[:, 2], 100), a.repeats)
    row = {"traces": a.traces, "length": a.length, "call_ms_best": best, "call_ms_median": med, "planning_ms": plan_best,
           "traces_per_s": a.traces / (best * 1e-3)}
    if not a.no_host:
        t0 = time.perf_counter()
        want = np.stack([A.trace_attributes(waves[i], p[i], s[i])[0] for i in range(a.traces)])
        host_ms = (time.perf_counter() - t0) * 1e3
        row.update(host_ms=host_ms, speedup=host_ms / best, worst_fi_diff=_worst(cols["trace_frequency_index"], want[:, 3]),
                   worst_mean_snr_diff=_worst(cols["trace_mean_snr_db"], want[:, 13]))
    bank.close()
    result["bank"] = row

    # ---- 2. the picks of a station-day
    n_day = int(a.hours * 3600 * 100)
    x, _, _ = synthetic_stream_array(n_day, seed=7)
    x = (x * 2000.0 + 1234.0).astype(np.float32)  # counts with an offset
    t0_ = va.UTCDateTime("2021-03-01T00:00:00")
    host_stream = va.Stream([va.Trace(x[c], {"network": "XX", "station": "DAY", "location": "", "channel": "HH" + comp,
                                             "starttime": t0_, "sampling_rate": 100.0}) for c, comp in enumerate("ZNE")])
    moved = va.to_device(host_stream)
    model = va.PhaseNet.from_pretrained("volpick").cuda()
    picks = list(model.classify(moved).picks)
    row = {"hours": a.hours, "samples": n_day, "picks": len(picks)}
    if picks:
        cols, best, med = _timed(lambda: va.pick_attributes(moved, picks), a.repeats)
        row.update(call_ms_best=best, call_ms_median=med, picks_per_s=len(picks) / (best * 1e-3))
        if not a.no_host:
            ks = [int(round((pk.peak_time - t0_) * 100.0)) for pk in picks]
            t0 = time.perf_counter()
            want = []
            for k in ks:
                lo = max(0, k - 700)
                want.append(A.trace_attributes(x[:, lo : k + 800], k - lo, None, demean=True)[0])
            host_ms = (time.perf_counter() - t0) * 1e3
            want = np.stack(want)
            row.update(host_ms=host_ms, speedup=host_ms / best, worst_fi_diff=_worst(cols["trace_frequency_index"], want[:, 3]),
                       worst_mean_snr_diff=_worst(cols["trace_mean_snr_db"], want[:, 13]))
    result["station_day_picks"] = row
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
