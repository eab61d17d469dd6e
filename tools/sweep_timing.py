#!/usr/bin/env python3
"""What the pick-benchmark task 0 costs on one MI355X, on a synthetic bank.

default   a PhaseNet pass over --windows steered targets (35,120: the reference's evaluation size) at batch 1024 and the
          reference's nine thresholds, --passes times, the three kinds of pass taking turns:
            sweep        ``evaluate.sweep_bank`` without values (the reference never saves scores): cut, normalise, forward
                         and sweep on the GPU, one host wait per pass, counts and peaks copied out;
            sweep+value  the same with the maxima kept and copied out;
            tasks 1-3    ``evaluate.predict_bank`` over the same windows: the pass the sweep pass is set against;
          then, once, the parent commit's way on the same windows, pre-cut on the host: ``evaluate_windows`` once per
          threshold (nine forward passes, eighteen ``vp_pick_windows`` launches per batch, a Python sort per window), with
          its picks compared against the sweep's (they must be equal).
--kernel  the sweep launch alone: --launches calls of ``vp_sweep_windows`` at B = 1024, NT = 9, K = 8, no values, on
          device-resident probabilities for both models, whole windows, in three groups of 10 + --launches launches:
            resident  probabilities the model's forward pass left (of synthetic windows), every launch on the same array,
                      which stays in the 256 MB Infinity Cache as a batch's probabilities do behind the forward pass;
            streamed  the launches rotating over copies of that array, 590 MB in all: each one reads its bytes from HBM;
            one run   an array whose every row is ONE run over the whole border at every threshold, resident.
          Each call also copies the counts and peaks back and waits, so its wall time is an upper bound; the kernel's own
          time is in the kernel trace of
            rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/sweep_timing.py --kernel
          (launch order: per model the three groups above), set against the byte floor printed here: the 2 T 4 B bytes
          read plus the bytes written, over the 6.29 TB/s of a float4 copy from HBM.  The wall time of a forward call of
          the same batch is printed beside it: what a whole-border run may not exceed.
usage: sweep_timing.py [--kernel] [--windows 35120] [--passes 10] [--launches 200]"""
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
from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s: the measured float4 copy rate of the MI355X's HBM
STREAMED_BYTES = 590_000_000  # more than twice the 256 MB Infinity Cache: a rotation over this much reads from HBM
GRID = np.arange(0.1, 1.0, 0.1)

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--windows", type=int, default=35_120)
ap.add_argument("--passes", type=int, default=10)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--traces", type=int, default=128)
args = ap.parse_args()
lib = _lib.load()
B = 1024
ptr = lambda a: a.ctypes.data_as(C.c_void_p)

if args.kernel:
    NT, K = 9, 8
    on, off, _ = E._sweep_grid(GRID)
    result = {}
    for cls in (PhaseNet, EQTransformer):
        model = cls.from_pretrained("volpick")
        model._max_batch = B
        model.cuda()
        T = model.in_samples
        p_row, s_row = E._sweep_rows(model)
        x = synthetic_windows(B, T, seed=1)
        x = x - x.mean(-1, keepdims=True)
        x = torch.from_numpy((x / (np.abs(x).max(-1, keepdims=True) + 1e-10)).astype(np.float32)).cuda()
        typical = model._forward_raw(x)
        n_read, n_written = 2 * T * 4 * B, 4 * B * 2 * NT * (1 + K)
        n_array = 3 * T * 4 * B
        streamed = [typical] + [typical.clone() for _ in range(-(-STREAMED_BYTES // n_array) - 1)]
        one_run = torch.full((B, 3, T), 0.95, device="cuda")
        count, peak = np.zeros((B, 2, NT), np.int32), np.zeros((B, 2, NT, K), np.int32)
        h = model._ensure_handle()
        torch.cuda.synchronize()

        def launch(prob):
            _lib.check(lib.vp_sweep_windows(h, C.c_void_p(prob.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, p_row, s_row, None, None,
                                            ptr(on), ptr(off), NT, K, ptr(count), ptr(peak), None))

        r = result[model.name] = {"B": B, "T": T, "NT": NT, "K": K, "bytes_read": n_read, "bytes_written": n_written,
                                  "byte_floor_us": 1e6 * (n_read + n_written) / COPY_RATE, "streamed_arrays": len(streamed)}
        for kind, arrays in (("resident", streamed[:1]), ("streamed", streamed), ("one_run", [one_run])):
            for i in range(10):
                launch(arrays[i % len(arrays)])
            t0 = time.perf_counter()
            for i in range(args.launches):
                launch(arrays[i % len(arrays)])
            r[f"call_wall_us_{kind}"] = 1e6 * (time.perf_counter() - t0) / args.launches
            r[f"triggers_per_window_{kind}"] = float(count.sum()) / B
        assert (count == 1).all() and (peak[..., 0] == 0).all() and (peak[..., 1:] == -1).all()  # one run each, its first sample
        for _ in range(3):
            model._forward_raw(x)
        t0 = time.perf_counter()
        for _ in range(20):
            model._forward_raw(x)  # (returns after its own host wait)
        r["forward_call_wall_us"] = 1e6 * (time.perf_counter() - t0) / 20
        print(f"{model.name}: reads {n_read / 1e6:.1f} MB, writes {n_written / 1e6:.2f} MB per launch, byte floor "
              f"{r['byte_floor_us']:.2f} us; vp_sweep_windows call (launch + {n_written / 1e3:.0f} KB back + wait) "
              f"{r['call_wall_us_resident']:.1f} us resident ({r['triggers_per_window_resident']:.1f} triggers per window), "
              f"{r['call_wall_us_streamed']:.1f} us streamed over {len(streamed)} arrays, {r['call_wall_us_one_run']:.1f} us "
              f"with one whole-border run per row; a forward call of the same batch {r['forward_call_wall_us']:.1f} us")
        del streamed, one_run, typical
    print(json.dumps({"sweep_kernel_timing": result}))
    sys.exit(0)

# ---- a pass at the reference's size ----------------------------------------------------------------------------------------
rng = np.random.default_rng(0)
L = 9000
waves = []
for i in range(args.traces):
    w, _, _ = synthetic_stream_array(L, seed=2000 + i, n_events=1)
    waves.append(w * rng.uniform(0.1, 100.0))
bank = G.WaveformBank(np.stack(waves).astype(np.float32), {})
model = PhaseNet.from_pretrained("volpick")
model._max_batch = B
model.cuda()
T = model.in_samples
n = args.windows
width = np.where(np.arange(n) % 2 == 0, 1000, 3000)  # 10 s and 30 s targets
start = (rng.random(n) * (L - width)).astype(np.int64)
targets = {"trace": rng.integers(0, args.traces, n), "start_sample": start, "end_sample": start + width}
rows, borders = G.SteeredPlanner(bank, T).plan(targets)
MAX_PICKS = 8

PASSES = {"sweep": lambda: E.sweep_bank(model, bank, rows, borders, GRID, B, MAX_PICKS),
          "sweep_value": lambda: E.sweep_bank(model, bank, rows, borders, GRID, B, MAX_PICKS, scores=True),
          "tasks123": lambda: E.predict_bank(model, bank, rows, borders, batch_size=B)}


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


while True:  # warm-up: scratch, code objects; and room for the busiest window of this bank
    try:
        for f in PASSES.values():
            f()
        break
    except RuntimeError:
        if MAX_PICKS >= E.SWEEP_MAX_PICKS:
            raise
        MAX_PICKS *= 2
times = {k: [] for k in PASSES}
got = None
for _ in range(args.passes):  # the three kinds in turn, so that a drifting clock meets them alike
    for k, f in PASSES.items():
        t, out = timed(f)
        times[k].append(t)
        if k == "sweep_value":
            got = out
count, peak, value = got


def parent_way():
    """``evaluate_windows`` once per threshold on the windows pre-cut on the host, as the parent commit sweeps."""
    X = np.concatenate([bank.make_batch(rows[b0:b0 + B], model, 20)["X"].cpu().numpy() for b0 in range(0, n, B)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    per_threshold = [E.evaluate_windows(model, X, borders, threshold=thr, batch_size=B, max_picks=64) for thr in GRID]
    return time.perf_counter() - t0, per_threshold


parent_s, per_threshold = parent_way()
same = True
for j, (pp, ps, sp, ss) in enumerate(per_threshold):
    for ph, (pk, sc) in enumerate(((pp, ps), (sp, ss))):
        same = same and all(np.array_equal(pk[i], peak[i, ph, j, :count[i, ph, j]]) and
                            np.array_equal(sc[i], value[i, ph, j, :count[i, ph, j]]) for i in range(n))
med = {k: float(np.median(v)) for k, v in times.items()}
result = {"windows": n, "batch": B, "thresholds": len(GRID), "max_picks": MAX_PICKS, "passes": args.passes,
          "pass_s": med, "pass_min_s": {k: min(v) for k, v in times.items()}, "pass_max_s": {k: max(v) for k, v in times.items()},
          "sweep_over_tasks123": med["sweep"] / med["tasks123"], "sweep_value_over_tasks123": med["sweep_value"] / med["tasks123"],
          "bytes_copied_out": {"sweep": int(count.nbytes + peak.nbytes), "sweep_value": int(count.nbytes + peak.nbytes + value.nbytes)},
          "triggers_per_window": float(count.sum()) / n, "parent_way_s": parent_s, "parent_over_sweep": parent_s / med["sweep"],
          "results_equal": bool(same)}
print(f"{n} windows at batch {B}, {len(GRID)} thresholds: sweep pass {1e3 * med['sweep']:.2f} ms (median of {args.passes}: "
      f"{1e3 * min(times['sweep']):.2f}-{1e3 * max(times['sweep']):.2f}), with values {1e3 * med['sweep_value']:.2f} ms, tasks 1-3 pass "
      f"{1e3 * med['tasks123']:.2f} ms ({1e3 * min(times['tasks123']):.2f}-{1e3 * max(times['tasks123']):.2f}): sweep / tasks 1-3 = "
      f"{result['sweep_over_tasks123']:.2f}; evaluate_windows once per threshold {parent_s:.2f} s: {result['parent_over_sweep']:.0f}x; "
      f"{result['triggers_per_window']:.2f} triggers per window; results equal: {same}")
bank.close()
print(json.dumps({"sweep_timing": result}))
sys.exit(0 if same else 1)
