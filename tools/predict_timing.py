#!/usr/bin/env python3
"""What the pick-benchmark tasks 1-3 cost on one MI355X (LOG.md), on a synthetic bank.

default   a PhaseNet pass over --windows steered targets (35,120: the reference's evaluation size) at batch 1024:
            device  ``evaluate.predict_bank``: cut, normalise, forward and reduce on the GPU, one host wait per pass: the
                    median of --passes passes timed one by one, and --passes passes back to back in one timed window;
            host    the reference's protocol on the same windows: per batch ``bank.make_batch`` -> ``_forward_raw`` -> copy
                    back -> the per-window loop of ``predict_step`` (five torch reductions per window) on one host thread;
          and the two results compared (they must be equal).
--kernel  the reduction alone: --launches calls of ``vp_predict_windows`` at B = 1024 on device-resident probabilities for
          both models, whole windows, twice: "resident", every launch on the same array (36.9 / 73.7 MB: it stays in the
          256 MB Infinity Cache), then "streamed", the launches rotating over arrays of 590 MB in all, so that each one reads
          its bytes from HBM.  Each call also copies 20 KB of records back and waits, so its wall time is an upper bound; the
          kernel's own time is in the kernel trace of
            rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/predict_timing.py --kernel
          (launch order: per model 10 + --launches resident, then 10 + --launches streamed), set against the byte floor
          printed here: 3 T 4 B bytes over the 6.29 TB/s of a float4 copy from HBM -- the floor of the streamed launches.
usage: predict_timing.py [--kernel] [--windows 35120] [--passes 30] [--launches 200]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from volpick_amd import EQTransformer, PhaseNet, _lib  # noqa: E402
from volpick_amd import evaluate as E  # noqa: E402
from volpick_amd import generate as G  # noqa: E402
from volpick_amd.synthetic import synthetic_stream_array  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s: the measured float4 copy rate of the MI355X's HBM
STREAMED_BYTES = 590_000_000  # more than twice the 256 MB Infinity Cache: a rotation over this much reads from HBM

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--windows", type=int, default=35_120)
ap.add_argument("--passes", type=int, default=30)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--traces", type=int, default=128)
args = ap.parse_args()
lib = _lib.load()
B = 1024

if args.kernel:
    result = {}
    for cls in (PhaseNet, EQTransformer):
        model = cls.from_pretrained("volpick").cuda()
        T = model.in_samples
        det_row, p_row, s_row, mode = E._predict_rows(model)
        n_bytes = 3 * T * 4 * B
        probs = [torch.rand((B, 3, T), device="cuda") for _ in range(-(-STREAMED_BYTES // n_bytes))]
        rec = np.zeros(B, E.RECORD)
        h = model._ensure_handle()
        torch.cuda.synchronize()

        def launch(prob):
            _lib.check(lib.vp_predict_windows(h, C.c_void_p(prob.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, det_row, p_row, s_row, mode,
                                              None, None, rec.ctypes.data_as(C.c_void_p)))

        r = result[model.name] = {"B": B, "T": T, "bytes_read": n_bytes, "byte_floor_us": 1e6 * n_bytes / COPY_RATE,
                                  "streamed_arrays": len(probs)}
        for kind, arrays in (("resident", probs[:1]), ("streamed", probs)):
            for i in range(10):
                launch(arrays[i % len(arrays)])
            t0 = time.perf_counter()
            for i in range(args.launches):
                launch(arrays[i % len(arrays)])
            r[f"call_wall_us_{kind}"] = 1e6 * (time.perf_counter() - t0) / args.launches
        print(f"{model.name}: {n_bytes / 1e6:.1f} MB per launch, byte floor {r['byte_floor_us']:.2f} us, vp_predict_windows call "
              f"(launch + 20 KB back + wait) {r['call_wall_us_resident']:.1f} us resident, {r['call_wall_us_streamed']:.1f} us "
              f"streamed over {len(probs)} arrays")
    print(json.dumps({"predict_kernel_timing": result}))
    sys.exit(0)

# ---- a pass at the reference's size ----------------------------------------------------------------------------------------
rng = np.random.default_rng(0)
L = 9000
waves = []
for i in range(args.traces):
    x, _, _ = synthetic_stream_array(L, seed=2000 + i, n_events=1)
    waves.append(x * rng.uniform(0.1, 100.0))
bank = G.WaveformBank(np.stack(waves).astype(np.float32), {})
model = PhaseNet.from_pretrained("volpick")
model._max_batch = B
model.cuda()
T = model.in_samples
n = args.windows
width = np.where(np.arange(n) % 2 == 0, 1000, 3000)  # task 2-3 (10 s) and task 1 (30 s) targets
start = (rng.random(n) * (L - width)).astype(np.int64)
targets = {"trace": rng.integers(0, args.traces, n), "start_sample": start, "end_sample": start + width}
rows, borders = G.SteeredPlanner(bank, T).plan(targets)


def device_pass():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = E.predict_bank(model, bank, rows, borders, batch_size=B)
    return time.perf_counter() - t0, out


def host_pass():
    """predict_step as the reference runs it (volpick/model/models.py:454-480), the windows from the same bank."""
    torch.set_num_threads(1)
    noise, p_id, s_id = model.labels.index("N"), model.labels.index("P"), model.labels.index("S")
    out = [torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=int), torch.zeros(n, dtype=int)]
    parts = {"forward_s": 0.0, "copy_back_s": 0.0, "loop_s": 0.0}
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for b0 in range(0, n, B):
        t0 = time.perf_counter()
        x = bank.make_batch(rows[b0:b0 + B], model, 20)["X"]
        y = model._forward_raw(x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pred = y.cpu()
        t2 = time.perf_counter()
        for i in range(pred.shape[0]):
            a, e = borders[b0 + i]
            local = pred[i, :, a:e]
            out[0][b0 + i] = torch.max(1 - local[noise])
            out[1][b0 + i] = torch.max(local[p_id]) / torch.max(local[s_id])
            out[2][b0 + i] = torch.argmax(local[p_id])
            out[3][b0 + i] = torch.argmax(local[s_id])
        t3 = time.perf_counter()
        parts["forward_s"] += t1 - t0
        parts["copy_back_s"] += t2 - t1
        parts["loop_s"] += t3 - t2
    return time.perf_counter() - t_all, [o.numpy() for o in out], parts


device_pass()  # warm-up: scratch, code objects
times, got = [], None
for _ in range(args.passes):
    t, got = device_pass()
    times.append(t)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.passes):  # one timed window of about half a second
    E.predict_bank(model, bank, rows, borders, batch_size=B)
back_to_back_s = (time.perf_counter() - t0) / args.passes
host_s, want, parts = host_pass()
same = all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
dev_s = float(np.median(times))
result = {"windows": n, "batch": B, "passes": args.passes, "device_pass_s": dev_s, "device_pass_min_s": min(times),
          "device_pass_max_s": max(times), "device_pass_back_to_back_s": back_to_back_s, "device_us_per_window": 1e6 * dev_s / n,
          "host_pass_s": host_s, "host_parts_s": parts, "host_over_device": host_s / dev_s, "results_equal": bool(same),
          "bytes_not_copied_back": int(n) * 3 * T * 4}
print(f"{n} windows at batch {B}: device pass {1e3 * dev_s:.2f} ms (median of {args.passes}: {1e3 * min(times):.2f}-{1e3 * max(times):.2f}; "
      f"{1e3 * back_to_back_s:.2f} ms per pass in one window of {args.passes}; {1e6 * dev_s / n:.3f} us per window), host protocol {host_s:.3f} s "
      f"(forward {parts['forward_s']:.3f}, copy back {parts['copy_back_s']:.3f}, loop {parts['loop_s']:.3f}): "
      f"{host_s / dev_s:.1f}x; results equal: {same}")
bank.close()
print(json.dumps({"predict_timing": result}))
sys.exit(0 if same else 1)
