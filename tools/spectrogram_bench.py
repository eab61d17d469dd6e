"""Device spectrogram (vp_spectrogram) of one component of a 100 Hz station-day (8.64 M int32 counts resident in HBM) at the
reference's defaults (nfft 128, pad 1024, hop 13: 664,606 frames of 512 bins, 1.36 GB of float32):

  * vp_spectrogram_bench: HIP events around `iters` repetitions of the whole call (mean pass, tables, frame kernel) after two
    untimed ones, and of the frame kernel alone; the whole day in one launch, or in `--pieces` frame ranges into one buffer
    of a piece's size;
  * the write floor: the output's bytes at the copy rate of BASELINE.md (6.29 TB/s);
  * the host path it replaces, as a device-resident caller pays it: .cpu() of the day, then matplotlib's mlab.specgram plus
    the reference's lines behind it (the numpy restatement of tests/spectrogram_f64.py where matplotlib is absent) on a
    `--slice-minutes` SLICE of the day, one thread; the day's figure is that time scaled by the frame counts, and is
    reported as an extrapolation.

    python tools/spectrogram_bench.py [--iters 5] [--hours 24] [--pieces 1] [--slice-minutes 10] [--out profiles/spectrogram.json]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
COPY_RATE = 6.29e12  # bytes per second, BASELINE.md


def host_slice(x, rate):
    """(seconds, what ran, the slice's amplitude spectrogram) of the host path on the samples `x`."""
    t0 = time.perf_counter()
    try:
        from matplotlib import mlab

        y = x - x.mean()
        spec, _, _ = mlab.specgram(y, Fs=rate, NFFT=128, pad_to=1024, noverlap=115)
        spec = np.sqrt(spec[1:, :])
        what = "matplotlib.mlab.specgram"
    except ImportError:
        from tests.spectrogram_f64 import spectrogram_f64

        spec = spectrogram_f64(x, rate)[0]
        what = "numpy restatement (tests/spectrogram_f64.py)"
    return time.perf_counter() - t0, what, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--hours", type=float, default=24.0)
    ap.add_argument("--pieces", type=int, default=1)
    ap.add_argument("--slice-minutes", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(HERE))
    import torch

    from volpick_amd import _lib
    from volpick_amd import spectrogram as VS

    lib = _lib.load()
    rate = 100.0
    n = int(3600 * rate * a.hours)
    rng = np.random.default_rng(100)
    x = np.round(800.0 * rng.standard_normal(n) + 30000.0 * np.sin(np.arange(n) / 5000.0) + 123456.0).astype(np.int32)
    d = torch.from_numpy(x).cuda()
    nfft, pad, _, hop, n_frames = VS.plan(n, rate)
    per_piece = -(-n_frames // a.pieces)
    out = torch.empty((pad // 2, per_piece), dtype=torch.float32, device="cuda")
    result = {"device": torch.cuda.get_device_name(0), "samples": n, "nfft": nfft, "pad": pad, "hop": hop, "frames": n_frames,
              "pieces": a.pieces, "iters": a.iters, "output_bytes": n_frames * (pad // 2) * 4}

    total_ms = frames_ms = 0.0
    for first in range(0, n_frames, per_piece):
        count = min(per_piece, n_frames - first)
        ms, ms_f = C.c_float(0), C.c_float(0)
        torch.cuda.synchronize()
        _lib.check(lib.vp_spectrogram_bench(0, d.data_ptr(), _lib.VP_SAMPLES_INT32, 1, n, n, rate, nfft, pad, hop, 0, first, count,
                                            out.data_ptr(), a.iters, C.byref(ms), C.byref(ms_f)), "vp_spectrogram_bench")
        total_ms += ms.value
        frames_ms += ms_f.value
    floor_ms = result["output_bytes"] / COPY_RATE * 1e3
    # per frame and residue: nfft-point complex transform, 5 nfft log2(nfft) flop; ratio / 2 + 1 residues
    flop = n_frames * (pad // nfft // 2 + 1) * 5.0 * nfft * np.log2(nfft)
    result.update({"device_ms": total_ms, "frame_kernel_ms": frames_ms, "write_floor_ms": floor_ms,
                   "over_write_floor": total_ms / floor_ms, "achieved_write_GBps": result["output_bytes"] / (total_ms * 1e-3) / 1e9,
                   "transform_gflop": flop / 1e9, "transform_tflops": flop / (frames_ms * 1e-3) / 1e12})

    t0 = time.perf_counter()  # one whole call as a caller sees it
    got = VS.spectrogram(d, rate, frames=(0, min(per_piece, n_frames)))
    result["call_wall_ms"] = (time.perf_counter() - t0) * 1e3

    # the host path, on a slice
    m = min(n, int(a.slice_minutes * 60 * rate))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = d.cpu().numpy()
    t_d2h = time.perf_counter() - t0
    t_host, what, spec = host_slice(h[:m].astype(np.float64), rate)
    slice_frames = spec.shape[1]
    # the slice's own mean differs from the day's: compare the device on the same slice
    dev_slice = VS.spectrogram(d[:m], rate).data.cpu().numpy()
    result.update({"host_path": what, "host_slice_minutes": m / rate / 60.0, "host_slice_frames": slice_frames,
                   "host_slice_ms": t_host * 1e3, "host_d2h_day_ms": t_d2h * 1e3,
                   "host_day_ms_extrapolated_from_the_slice": t_d2h * 1e3 + t_host * 1e3 * n_frames / slice_frames,
                   "slice_max_rel_diff_device_vs_host": float(np.abs(dev_slice - spec).max() / np.abs(spec).max())})
    result["speedup_vs_host_extrapolated"] = result["host_day_ms_extrapolated_from_the_slice"] / total_ms
    del got
    result["scratch_bytes_released"] = VS.release_spectrogram_scratch(0)
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
