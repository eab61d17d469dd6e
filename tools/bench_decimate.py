"""Device decimation (vp_decimate_lowpass) on one component of a station-day at 200, 500 and 1000 Hz, int32 counts resident
in HBM (vp_decimate_lowpass_bench: HIP events around `iters` repetitions of both passes after three untimed ones), next to
the host path (volpick_amd.resample.resample_array, scipy, one core) on the same array and the same machine, and the
end-to-end classify(read(buf, device_resident=True)) of a 200 Hz three-component station-day.

    python tools/bench_decimate.py [--rates 200 500 1000] [--iters 20] [--hours 24] [--out profiles/decimate.json]
    python tools/bench_decimate.py --e2e-only --repo /path/to/another/checkout     # the same call on another commit

--e2e-only touches only read() and classify(), so the file can be pointed at a built checkout of an earlier commit (--repo)
to time the same call there.  The file of the end-to-end case holds plain int32 records (encoding 3): packing a 200 Hz
station-day into Steim-2 frames with the Python encoder takes many minutes, and the decode is not what is measured here.
"""
import argparse
import ctypes as C
import json
import struct
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]


def station_day_file(OM, three_component, rate, hours):
    rng = np.random.default_rng(8)
    hour = int(3600 * rate)
    parts = []
    for t in three_component(hour, rng, spikes=False, rate=rate):
        blob0 = OM.write_mseed([t], reclen=4096, encoding=OM.ENC_INT32)
        recs = OM.scan_records(blob0)
        for h in range(hours):
            blob = bytearray(blob0)
            for rec in recs:
                y, doy, hh, mm, ss, fr, _ = OM.us_to_btime(rec["start_us"] + h * 3_600_000_000)
                struct.pack_into(">HHBBBBH", blob, rec["offset"] + 20, y, doy, hh, mm, ss, 0, fr)
            parts.append(bytes(blob))
    return b"".join(parts)


def end_to_end(va, torch, buf, model_names, repeats):
    out = {}
    for name in model_names:
        model = getattr(va, name).from_pretrained("volpick").cuda()
        times, n_picks = [], 0
        for _ in range(repeats + 1):  # the first call is the warm-up (plan, scratch, allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = va.read(buf, device_resident=True)
            t1 = time.perf_counter()
            n_picks = len(model.classify(st).picks)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            times.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
            on_device = all(getattr(tr, "_data", None) is None for tr in st)
        best = min(times[1:])
        out[name] = {"wall_ms": best[0], "read_ms": best[1], "classify_ms": best[2], "picks": n_picks,
                     "all_wall_ms": [round(t[0], 2) for t in times[1:]], "input_traces_never_copied_to_host": on_device}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=int, nargs="*", default=[200, 500, 1000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hours", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--models", nargs="*", default=["PhaseNet", "EQTransformer"])
    ap.add_argument("--e2e-only", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--repo", default=str(HERE), help="checkout to import volpick_amd from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.repo).resolve()))
    import torch

    import volpick_amd as va
    from oracle import mseed as OM  # input generator only
    from tests.mseed_util import three_component

    result = {"repo": str(Path(a.repo).resolve()), "device": torch.cuda.get_device_name(0)}
    if not a.e2e_only:
        from volpick_amd import _lib
        from volpick_amd.resample import lowpass_sos, resample_array

        lib = _lib.load()
        rows = []
        for rate in a.rates:
            k = rate // 100
            n = 86_400 * rate
            rng = np.random.default_rng(rate)
            x = np.round(800.0 * rng.standard_normal(n) + 30000.0 * np.sin(np.arange(n) / 5000.0) + 123456.0).astype(np.int32)
            d = torch.from_numpy(x).cuda()
            out = torch.empty((n + k - 1) // k, dtype=torch.float32, device="cuda")
            sos = np.ascontiguousarray(lowpass_sos(50.0, float(rate)))
            ms, ms_f = C.c_float(0), C.c_float(0)
            torch.cuda.synchronize()
            _lib.check(lib.vp_decimate_lowpass_bench(0, d.data_ptr(), _lib.VP_SAMPLES_INT32, n,
                                                     sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos), k, out.data_ptr(),
                                                     out.shape[0], a.iters, C.byref(ms), C.byref(ms_f)), "vp_decimate_lowpass_bench")
            t0 = time.perf_counter()  # one whole call as a caller sees it: scratch in place, launch, synchronise
            _lib.check(lib.vp_decimate_lowpass(0, d.data_ptr(), _lib.VP_SAMPLES_INT32, n, sos.ctypes.data_as(C.POINTER(C.c_double)),
                                               len(sos), k, out.data_ptr(), out.shape[0]), "vp_decimate_lowpass")
            t_call = time.perf_counter() - t0
            got = out.cpu().numpy()
            t0 = time.perf_counter()
            want = resample_array(x, float(rate), 100.0)
            t_host = time.perf_counter() - t0
            err = float(np.abs(got - want).max()) / (2.0 ** -22 * float(np.abs(x).max()))
            nbytes = n * (4 + 8 + 8) + 4 * out.shape[0]
            rows.append({"rate_hz": rate, "factor": k, "samples": n, "device_ms": ms.value, "forward_ms": ms_f.value,
                         "backward_ms": ms.value - ms_f.value, "call_wall_ms": t_call * 1e3, "host_ms": t_host * 1e3,
                         "speedup": t_host * 1e3 / ms.value, "algorithmic_bytes": nbytes,
                         "achieved_GBps": nbytes / (ms.value * 1e-3) / 1e9, "frac_of_8TBps": nbytes / (ms.value * 1e-3) / 8e12,
                         "worst_err_over_bound": err})
            del d, out
        freed = C.c_size_t(0)
        _lib.check(lib.vp_decimate_release_scratch(0, C.byref(freed)))
        result["component_day"] = rows
        result["scratch_bytes_released"] = int(freed.value)
    if not a.no_e2e:
        buf = station_day_file(OM, three_component, 200.0, a.hours)
        result["end_to_end_200hz_station_day"] = dict(end_to_end(va, torch, buf, a.models, a.repeats), file_bytes=len(buf),
                                                      hours=a.hours)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
