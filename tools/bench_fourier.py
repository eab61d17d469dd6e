"""Device Fourier resampling (vp_resample_fourier) on one component of a station-day at 250, 50 and 40 Hz, int32 counts resident
in HBM (vp_resample_fourier_bench: HIP events around `iters` repetitions of the whole conversion after three untimed ones, and
of the forward transform alone), next to the host path (volpick_amd.resample.resample_array, scipy, one core) on the same
array and the same machine, and the end-to-end classify(read(buf, device_resident=True)) of a 250 Hz three-component
station-day.

    python tools/bench_fourier.py [--rates 250 50 40] [--iters 10] [--hours 24] [--out profiles/fourier.json]
    python tools/bench_fourier.py --e2e-only --repo /path/to/another/checkout     # the same call on another commit

--e2e-only touches only read() and classify(), so the file can be pointed at a built checkout of an earlier commit (--repo)
to time the same call there (where the three components go through scipy on the host).  The file holds plain int32 records,
as in tools/bench_decimate.py, whose file builder and end-to-end loop this tool shares.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_decimate import end_to_end, station_day_file  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=int, nargs="*", default=[250, 50, 40])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hours", type=int, default=24)
    ap.add_argument("--short-by", type=int, default=0, help="samples missing from the component-day (an awkward length)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--models", nargs="*", default=["PhaseNet", "EQTransformer"])
    ap.add_argument("--e2e-only", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the host path's timing (and the error figure with it)")
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
        from volpick_amd.resample import fourier_args, resample_array

        lib = _lib.load()
        rows = []
        for rate in a.rates:
            n = a.hours * 3600 * rate - a.short_by
            num, df, dlf = fourier_args(n, float(rate), 100.0)
            rng = np.random.default_rng(rate)
            x = np.round(800.0 * rng.standard_normal(n) + 30000.0 * np.sin(np.arange(n) / 5000.0) + 123456.0).astype(np.int32)
            d = torch.from_numpy(x).cuda()
            out = torch.empty(num, dtype=torch.float32, device="cuda")
            args = (0, d.data_ptr(), _lib.VP_SAMPLES_INT32, n, float(rate), 100.0, num, df, dlf, out.data_ptr(), num)
            ms, ms_f = C.c_float(0), C.c_float(0)
            torch.cuda.synchronize()
            _lib.check(lib.vp_resample_fourier_bench(*args, a.iters, C.byref(ms), C.byref(ms_f)), "vp_resample_fourier_bench")
            t0 = time.perf_counter()  # one whole call as a caller sees it: scratch in place, launches, synchronise
            _lib.check(lib.vp_resample_fourier(*args), "vp_resample_fourier")
            t_call = time.perf_counter() - t0
            row = {"rate_hz": rate, "samples": n, "out_samples": num, "device_ms": ms.value, "forward_ms": ms_f.value,
                   "inverse_ms": ms.value - ms_f.value, "call_wall_ms": t_call * 1e3}
            if not a.no_host:
                got = out.cpu().numpy()
                t0 = time.perf_counter()
                want = resample_array(x, float(rate), 100.0)
                t_host = time.perf_counter() - t0
                row.update(host_ms=t_host * 1e3, speedup=t_host * 1e3 / ms.value,
                           worst_err_over_bound=float(np.abs(got - want).max()) / (2.0 ** -22 * float(np.abs(x).max())))
            rows.append(row)
            del d, out
        freed = C.c_size_t(0)
        _lib.check(lib.vp_resample_release_scratch(0, C.byref(freed)))
        result["component_day"] = rows
        result["scratch_bytes_released"] = int(freed.value)
    if not a.no_e2e:
        buf = station_day_file(OM, three_component, 250.0, a.hours)
        result["end_to_end_250hz_station_day"] = dict(end_to_end(va, torch, buf, a.models, a.repeats), file_bytes=len(buf),
                                                      hours=a.hours)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
