"""What writing miniSEED from a device-resident trace costs: one component of a 100 Hz station-day (8.64 M int32 samples, the
committed six-minute fixture's samples tiled), Steim-2 at 512 and 4096 bytes and float32 at 4096.

Per case: the kernel time of every stage (vp_mseed_encode_bench: HIP events, mean of --iters launches after 3 warm-up
launches of that stage); the byte floor of the whole encode, (4 bytes read per sample + file bytes written) / HBM rate; the
end-to-end ``write_mseed`` to ``bytes`` (host clock around a call that ends in a synchronise: two warm-up calls, then
--repeats calls, median and spread); and, in the same run and taking turns with it, what a user pays today before any
writer can start -- ``trace.data`` of the same trace, the device-to-host copy of 4 bytes per sample.

    python tools/mseed_write_timing.py [--iters 20] [--repeats 7] [--cases steim2-512,steim2-4096,float32-4096] [--out FILE]
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from volpick_amd import _lib, write_mseed  # noqa: E402
from volpick_amd.stream import Trace, UTCDateTime  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12  # bytes/s: a float4 copy on this part, and the data sheet
STAGES = ("classify", "chunk maps", "compose", "emit", "pack", "plain")


def device_trace(x):
    return Trace(header=dict(network="XX", station="VOLC", location="", channel="HHZ", starttime=UTCDateTime(1_600_000_000.0),
                             sampling_rate=100.0), device_data=x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="steim2-512,steim2-4096,float32-4096", help="which cases, in which order")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mseed_write_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    six = np.load(ROOT / "tests" / "golden" / "bench_steim2_6min_samples.npz")["HHZ"].astype(np.int32)
    day = np.tile(six, 8_640_000 // len(six))
    lib = _lib.load()
    lines = [f"one component of a station-day: {len(day)} samples at 100 Hz ({len(six)} fixture samples x {len(day) // len(six)}), "
             f"{torch.cuda.get_device_name(0)}",
             f"kernel times: HIP events, mean of {a.iters} launches per stage after 3 warm-up launches; end to end: host clock, "
             f"median [min .. max] of {a.repeats} calls after 2 warm-up calls, write_mseed and trace.data taking turns", ""]
    cases = {"steim2-512": ("Steim-2, 512-byte records", day, 11, 512), "steim2-4096": ("Steim-2, 4096-byte records", day, 11, 4096),
             "float32-4096": ("float32, 4096-byte records", day.astype(np.float32), 4, 4096)}
    for name, samples, encoding, reclen in (cases[k] for k in a.cases.split(",")):
        x = torch.from_numpy(samples).cuda()
        t = _lib.VpMseedTrace()
        t.start_us, t.sample_rate, t.first_sample, t.nsamples, t.quality = 1_600_000_000_000_000, 100.0, 0, len(samples), ord("D")
        t.network, t.station, t.channel = b"XX", b"VOLC", b"HHZ"
        ms = (C.c_float * _lib.VP_MSEED_ENCODE_STAGES)()
        kind = _lib.VP_SAMPLES_INT32 if encoding == 11 else _lib.VP_SAMPLES_FLOAT32
        torch.cuda.synchronize()
        _lib.check(lib.vp_mseed_encode_bench(0, C.c_void_p(x.data_ptr()), kind, C.byref(t), 1, reclen, encoding, 1, a.iters, ms),
                   "vp_mseed_encode_bench")
        t_write, t_data, nbytes = [], [], 0
        for k in range(a.repeats + 2):
            tr = device_trace(x)
            t0 = time.perf_counter()
            blob = write_mseed(tr, reclen=reclen, encoding=encoding)
            t1 = time.perf_counter()
            host = device_trace(x).data  # a fresh trace: the copy is made, not remembered
            t2 = time.perf_counter()
            assert tr._data is None and len(host) == len(samples)
            nbytes = len(blob)
            if k >= 2:
                t_write.append((t1 - t0) * 1e3)
                t_data.append((t2 - t1) * 1e3)
        kernels = sum(ms)
        floor_bytes = 4 * len(samples) + nbytes
        lines.append(f"{name}: {nbytes} file bytes ({nbytes / len(samples):.3f} per sample, {nbytes // reclen} records)")
        for stage, v in zip(STAGES, ms):
            if v > 0:
                lines.append(f"    {stage:<11}{v:9.4f} ms  ({100 * v / kernels:4.1f} % of the kernel time)")
        lines.append(f"    all kernels{kernels:8.4f} ms = {len(samples) / kernels / 1e6:.2f} G samples/s")
        lines.append(f"    byte floor  {floor_bytes / HBM_MEASURED * 1e3:8.4f} ms at {HBM_MEASURED / 1e12:.2f} TB/s measured copy rate "
                     f"({floor_bytes / HBM_SPEC * 1e3:.4f} ms at the {HBM_SPEC / 1e12:.0f} TB/s of the data sheet): the kernels take "
                     f"{kernels / (floor_bytes / HBM_MEASURED * 1e3):.1f} x the floor")
        for label, v in (("write_mseed -> bytes", t_write), ("trace.data (D2H copy)", t_data)):
            lines.append(f"    {label:<22}{statistics.median(v):9.2f} ms  [{min(v):.2f} .. {max(v):.2f}]")
        lines.append(f"    write_mseed / trace.data = {statistics.median(t_write) / statistics.median(t_data):.2f}; kernels / write_mseed = "
                     f"{kernels / statistics.median(t_write):.3f}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
