#!/usr/bin/env python3
"""What the STA/LTA check of the reference's waveform test costs on one MI355X ("STA/LTA triggers"): one component
and three components of a 100 Hz station-day (8.64 M float32 samples each, resident in HBM: noise with a burst every ten
minutes), nsta, nlta = 500, 2000 (5 s, 20 s), thresholds 2 and 0.5.

  * vp_sta_lta_bench, both types, float32 out: HIP events around --iters repetitions of the whole call after three untimed
    ones, set against the byte floor -- the bytes the scheme moves over the 6.29 TB/s of a float4 copy from HBM.  Recursive:
    the input twice (reduce, apply) and the output once, 12 bytes per sample.  Classic: the input three times (reduce, suffix,
    final), the two suffix arrays written and read as float64, the output once, 48 bytes per sample;
  * vp_sos_filter_bench, one pass, on the same trace (0.3 Hz high-pass, 2 sections; 1-20 Hz band-pass, 4 sections), once per
    component: the yardstick for a carry-scan kernel in this tree;
  * vp_trigger_onset on the float32 cft the recursive type left: a host clock around --iters whole calls (row table up, scan,
    result block back, wait, sort), there being no device-event entry for it;
  * volpick_amd.sta_lta_triggers on the device-resident stream: a host clock around the whole public call;
  * the host path a device-resident caller pays without all this: .cpu(), the numpy / lfilter restatement, the host trigger
    mirror, per component; the triggers of both paths are compared.

    python tools/stalta_timing.py [--iters 20] [--hours 24] [--out profiles/stalta_timing.txt]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
COPY_RATE = 6.29e12  # bytes/s: the measured float4 copy rate of the MI355X's HBM
NSTA, NLTA, THR_ON, THR_OFF = 500, 2000, 2.0, 0.5
FLOOR_BYTES = {"recstalta": 4 + 4 + 4, "classicstalta": 3 * 4 + 2 * (8 + 8) + 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hours", type=int, default=24)
    ap.add_argument("--out", default=str(HERE / "profiles" / "stalta_timing.txt"))
    a = ap.parse_args()
    sys.path.insert(0, str(HERE))
    import torch

    import volpick_amd as va
    from volpick_amd import _lib, trigger as TR
    from volpick_amd.signal import butter_sos

    lib = _lib.load()
    n = 3600 * 100 * a.hours
    rng = np.random.default_rng(100)
    x = (800.0 * rng.standard_normal((3, n))).astype(np.float32)
    for at in range(30_000, n - 3000, 60_000):
        x[:, at:at + 3000] *= 8.0
    d = torch.from_numpy(x).cuda()
    out = torch.empty((3, n), dtype=torch.float32, device="cuda")
    lines = [f"tools/stalta_timing.py --iters {a.iters} --hours {a.hours} on {torch.cuda.get_device_name(0)}: {n} float32 samples per "
             f"component, nsta, nlta = {NSTA}, {NLTA}, thresholds {THR_ON}, {THR_OFF}"]
    result = {"device": torch.cuda.get_device_name(0), "samples": n, "iters": a.iters}

    def say(s):
        print(s)
        lines.append(s)

    for comps in (1, 3):
        r = result[f"components_{comps}"] = {}
        for name, code in TR.TYPES.items():
            ms = C.c_float(0)
            torch.cuda.synchronize()
            _lib.check(lib.vp_sta_lta_bench(0, C.c_void_p(d.data_ptr()), _lib.VP_SAMPLES_FLOAT32, comps, n, n, code, NSTA, NLTA,
                                            C.c_void_p(out.data_ptr()), _lib.VP_SAMPLES_FLOAT32, a.iters, C.byref(ms)), "vp_sta_lta_bench")
            floor = 1e3 * comps * n * FLOOR_BYTES[name] / COPY_RATE
            r[name] = {"device_ms": ms.value, "byte_floor_ms": floor, "over_floor": ms.value / floor,
                       "achieved_GBps": comps * n * FLOOR_BYTES[name] / (ms.value * 1e-3) / 1e9}
            say(f"{comps} component(s) {name}: {ms.value:.4f} ms per call; byte floor {floor:.4f} ms ({FLOOR_BYTES[name]} B per sample "
                f"at 6.29 TB/s): {ms.value / floor:.2f} x the floor")
        for fname, kind, opts in (("highpass 0.3 Hz", "highpass", dict(freq=0.3)), ("bandpass 1-20 Hz", "bandpass", dict(freqmin=1.0, freqmax=20.0))):
            sos = np.ascontiguousarray(butter_sos(kind, 100.0, **opts))
            total = 0.0
            for k in range(comps):
                ms = C.c_float(0)
                torch.cuda.synchronize()
                _lib.check(lib.vp_sos_filter_bench(0, C.c_void_p(d[k].data_ptr()), _lib.VP_SAMPLES_FLOAT32, n,
                                                   sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos), 0, C.c_void_p(out[k].data_ptr()),
                                                   a.iters, C.byref(ms), None), "vp_sos_filter_bench")
                total += ms.value
            r[f"sos_filter {fname}"] = {"sections": len(sos), "device_ms": total}
            say(f"{comps} component(s) vp_sos_filter one pass, {fname} ({len(sos)} sections): {total:.4f} ms; recstalta / filter = "
                f"{r['recstalta']['device_ms'] / total:.2f}")
        # the trigger scan on the recursive cft
        cft = TR.sta_lta_device(d[:comps], "recstalta", NSTA, NLTA, torch.float32)
        res = TR.trigger_onset_device(cft, THR_ON, THR_OFF)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            TR.trigger_onset_device(cft, THR_ON, THR_OFF)
        t_scan = 1e3 * (time.perf_counter() - t0) / a.iters
        r["trigger_onset"] = {"call_wall_ms": t_scan, "triggers": int(len(res[0]))}
        say(f"{comps} component(s) vp_trigger_onset (whole call, host clock): {t_scan:.4f} ms, {len(res[0])} triggers")
        hdr = dict(network="XX", station="DAY", sampling_rate=100.0)
        st = va.Stream([va.Trace(header=dict(hdr, channel="HH" + "ZNE"[k]), device_data=d[k]) for k in range(comps)])
        got = va.sta_lta_triggers(st, "recstalta", NSTA / 100.0, NLTA / 100.0, THR_ON, THR_OFF)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            got = va.sta_lta_triggers(st, "recstalta", NSTA / 100.0, NLTA / 100.0, THR_ON, THR_OFF)
        t_all = 1e3 * (time.perf_counter() - t0) / a.iters
        r["sta_lta_triggers"] = {"call_wall_ms": t_all}
        say(f"{comps} component(s) sta_lta_triggers (recstalta, whole public call, host clock): {t_all:.4f} ms")
        # the host path
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = d[:comps].cpu().numpy()
        t1 = time.perf_counter()
        cfts = [TR.recursive_sta_lta(h[k], NSTA, NLTA) for k in range(comps)]
        t2 = time.perf_counter()
        trig = [TR._pick_host(c.astype(np.float32), THR_ON, THR_OFF) for c in cfts]
        t3 = time.perf_counter()
        t_classic = time.perf_counter()
        TR.classic_sta_lta(h[0], NSTA, NLTA)
        t_classic = time.perf_counter() - t_classic
        same = all(np.array_equal(trig[k][0], got[st[k].id]["on"]) and np.array_equal(trig[k][1], got[st[k].id]["off"]) for k in range(comps))
        r["host_path"] = {"d2h_ms": 1e3 * (t1 - t0), "recursive_lfilter_ms": 1e3 * (t2 - t1), "trigger_mirror_ms": 1e3 * (t3 - t2),
                          "total_ms": 1e3 * (t3 - t0), "classic_cumsum_one_component_ms": 1e3 * t_classic, "triggers_equal": bool(same),
                          "over_sta_lta_triggers": 1e3 * (t3 - t0) / t_all}
        say(f"{comps} component(s) host path: .cpu() {1e3 * (t1 - t0):.1f} ms, lfilter restatement {1e3 * (t2 - t1):.1f} ms, host trigger "
            f"mirror {1e3 * (t3 - t2):.1f} ms, {1e3 * (t3 - t0):.1f} ms in all: {1e3 * (t3 - t0) / t_all:.0f} x sta_lta_triggers; classic "
            f"cumulative-sum restatement of one component {1e3 * t_classic:.1f} ms; on / off equal to the device's: {same}")
    result["scratch_bytes_released"] = TR.release_trigger_scratch(0)
    lines.append(json.dumps({"stalta_timing": result}))
    print(lines[-1])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
