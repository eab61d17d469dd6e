"""Device filter (vp_sos_filter) on one component of a 100 Hz station-day (8.64 M samples, int32 counts resident in HBM) for the
0.3 Hz high-pass (2 sections) and the 1-20 Hz band-pass (4 sections), one-pass and zero-phase:

  * vp_sos_filter_bench: HIP events around `iters` repetitions of the whole filter after three untimed ones, and of one pass's
    carry launch alone;
  * vp_decimate_lowpass_bench on the same trace (read as 200 Hz, factor 2: both passes, and the forward pass alone): the
    yardstick -- the same recursion once per sample, by warm-up, without a carry;
  * the host path for the same trace as a device-resident caller pays it: .cpu(), filter_array (scipy, one core), upload.

    python tools/filter_bench.py [--iters 20] [--hours 24] [--out profiles/filter.json]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
CASES = (("highpass 0.3 Hz", "highpass", dict(freq=0.3)), ("bandpass 1-20 Hz", "bandpass", dict(freqmin=1.0, freqmax=20.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hours", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(HERE))
    import torch

    from volpick_amd import _lib
    from volpick_amd.resample import lowpass_sos
    from volpick_amd.signal import butter_sos, filter_array

    lib = _lib.load()
    n = 3600 * 100 * a.hours
    rng = np.random.default_rng(100)
    x = np.round(800.0 * rng.standard_normal(n) + 30000.0 * np.sin(np.arange(n) / 5000.0) + 123456.0).astype(np.int32)
    d = torch.from_numpy(x).cuda()
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    dp = C.POINTER(C.c_double)
    result = {"device": torch.cuda.get_device_name(0), "samples": n, "iters": a.iters}

    sos = np.ascontiguousarray(lowpass_sos(50.0, 200.0))
    half = torch.empty((n + 1) // 2, dtype=torch.float32, device="cuda")
    ms, ms_f = C.c_float(0), C.c_float(0)
    torch.cuda.synchronize()
    _lib.check(lib.vp_decimate_lowpass_bench(0, d.data_ptr(), _lib.VP_SAMPLES_INT32, n, sos.ctypes.data_as(dp), len(sos), 2,
                                             half.data_ptr(), half.shape[0], a.iters, C.byref(ms), C.byref(ms_f)),
               "vp_decimate_lowpass_bench")
    result["decimate_yardstick"] = {"sections": len(sos), "both_passes_ms": ms.value, "forward_pass_ms": ms_f.value}

    rows = []
    for name, kind, opts in CASES:
        sos = np.ascontiguousarray(butter_sos(kind, 100.0, **opts))
        for zerophase in (0, 1):
            ms, ms_c = C.c_float(0), C.c_float(0)
            torch.cuda.synchronize()
            _lib.check(lib.vp_sos_filter_bench(0, d.data_ptr(), _lib.VP_SAMPLES_INT32, n, sos.ctypes.data_as(dp), len(sos),
                                               zerophase, out.data_ptr(), a.iters, C.byref(ms), C.byref(ms_c)), "vp_sos_filter_bench")
            t0 = time.perf_counter()  # one whole call as a caller sees it: table, scratch in place, launches, synchronise
            _lib.check(lib.vp_sos_filter(0, d.data_ptr(), _lib.VP_SAMPLES_INT32, n, sos.ctypes.data_as(dp), len(sos), zerophase,
                                         out.data_ptr()), "vp_sos_filter")
            t_call = time.perf_counter() - t0
            got = out.cpu().numpy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()  # the round trip the device path replaces
            h = d.cpu().numpy()
            t1 = time.perf_counter()
            want = filter_array(h, kind, 100.0, zerophase=bool(zerophase), **opts)
            t2 = time.perf_counter()
            up = torch.from_numpy(want.astype(np.float32)).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            del up
            passes = 2 if zerophase else 1
            # per pass: the input twice (reduce, apply) and the output once; the intermediate is float64
            nbytes = n * ((4 + 4 + 8) + (8 + 8 + 4) if zerophase else (4 + 4 + 4))
            rows.append({"filter": name, "sections": len(sos), "zerophase": bool(zerophase), "device_ms": ms.value,
                         "carry_launch_ms": ms_c.value, "carry_share": passes * ms_c.value / ms.value,
                         "call_wall_ms": t_call * 1e3, "host_total_ms": (t3 - t0) * 1e3, "host_d2h_ms": (t1 - t0) * 1e3,
                         "host_filter_ms": (t2 - t1) * 1e3, "host_h2d_ms": (t3 - t2) * 1e3,
                         "speedup_vs_host_round_trip": (t3 - t0) * 1e3 / ms.value,
                         "per_pass_over_decimate_forward": ms.value / passes / result["decimate_yardstick"]["forward_pass_ms"],
                         "algorithmic_bytes": nbytes, "achieved_GBps": nbytes / (ms.value * 1e-3) / 1e9,
                         "worst_err_over_bound": float(np.abs(got - want).max()) / (2.0 ** -22 * float(np.abs(x).max()))})
    result["station_day"] = rows
    freed = C.c_size_t(0)
    _lib.check(lib.vp_sos_filter_release_scratch(0, C.byref(freed)))
    result["scratch_bytes_released"] = int(freed.value)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
