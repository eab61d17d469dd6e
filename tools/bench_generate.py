"""GPU batch generation for PhaseNet training (volpick_amd/generate.py): the generation kernel alone, the fused training
step against the plain one with the batch already resident, and the host path it replaces.

    python tools/bench_generate.py [--batch 512] [--traces 2048] [--steps 40] [--rounds 3]
    python tools/bench_generate.py --kernel-only [--reps 200]       # under rocprofv3 --kernel-trace --stats
    python tools/bench_generate.py --augment [...]                  # AUG_ROW batches (AugmentedPlanner), both modes

``--augment`` plans with the reference's stacking, noise and gap probabilities (the bank's first three quarters as
event traces, the last quarter as noise traces), adds the planner's time per batch, and times the float64 numpy
restatement of the same records (tests/augment_restate.py) as the host path.

Prints one JSON line.  The bank holds synthetic 60 s three-component traces (6000 samples, one event each).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from volpick_amd import PhaseNet  # noqa: E402
from volpick_amd.generate import AugmentedPlanner, WaveformBank, WindowPlanner  # noqa: E402
from volpick_amd.synthetic import synthetic_stream_array  # noqa: E402
from volpick_amd.train import PhaseNetTrainer, gaussian_labels  # noqa: E402

SIGMA = 20.0


def make_bank_arrays(n, L=6000, seed=0):
    rng = np.random.default_rng(seed)
    w = np.empty((n, 3, L), np.float32)
    p = np.empty(n)
    s = np.empty(n)
    for i in range(n):
        x, pp, ss = synthetic_stream_array(L, seed=seed * 1000003 + i, n_events=1)
        w[i] = x * rng.uniform(0.1, 100.0)
        p[i], s[i] = pp[0], ss[0]
    return w, p, s


def host_batch(w_flat, L, onsets, rows, T=3001):
    """The host path: cut with zero fill, demean, peak-normalise, gaussian_labels (numpy, one thread)."""
    B = len(rows)
    t = np.arange(T)
    idx = rows["start"][:, None] + t[None, :]
    m = (idx >= rows["lo"][:, None]) & (idx < rows["hi"][:, None])
    base = rows["trace"].astype(np.int64)[:, None] * 3 * L
    x = np.empty((B, 3, T), np.float32)
    for c in range(3):
        x[:, c] = np.where(m, w_flat[base + c * L + np.where(m, idx, 0)], 0.0)
    x -= x.mean(-1, keepdims=True)
    x /= np.abs(x).max(-1, keepdims=True) + 1e-10
    st = rows["start"].astype(np.float64)
    y = gaussian_labels(onsets[rows["trace"], 0] - st, onsets[rows["trace"], 2] - st, T, SIGMA)
    return x, y


def time_loop(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--traces", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating step / step_bank rounds per dtype")
    ap.add_argument("--kernel-only", action="store_true", help="only the generation kernel, --reps times (for rocprofv3)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--augment", action="store_true", help="augmented rows (AugmentedPlanner) instead of block 1 alone")
    a = ap.parse_args()
    B = a.batch
    assert torch.cuda.is_available(), "bench_generate.py measures on the GPU"
    w, p, s = make_bank_arrays(a.traces)
    L = w.shape[2]
    bank = WaveformBank(w, {"P": p, "S": s})
    model = PhaseNet.from_pretrained("volpick")
    if a.augment:
        q = 3 * a.traces // 4
        planner = AugmentedPlanner(bank, B, np.arange(q), np.arange(q, a.traces), seed=1, sigma=SIGMA)
    else:
        planner = WindowPlanner(bank, B, seed=1)
    plans = [next(planner.epoch()) for _ in range(8)]
    out = {"metric": "PhaseNet training batches generated on the GPU", "batch": B, "traces": a.traces, "trace_samples": L,
           "norm": model.norm, "labels": model.labels, "augment": a.augment}
    if a.augment:
        t0 = time.perf_counter()
        for k in range(20):
            planner.plan(np.arange(k * B, (k + 1) * B) % a.traces)
        out["plan_ms_per_batch"] = (time.perf_counter() - t0) / 20 * 1e3
        ev = np.concatenate(plans)["event"]["kind"]
        out["event_entries_per_window"] = float((ev != 0).sum() / (len(plans) * B))

    # the kernel: one batch of B windows per launch
    for k in range(a.warmup):
        bank.make_batch(plans[k % 8], model, SIGMA)
    n = a.reps
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for k in range(n):
        bank.make_batch(plans[k % 8], model, SIGMA)
    ev1.record()
    torch.cuda.synchronize()
    per = ev0.elapsed_time(ev1) / n * 1e3
    moved = B * 3 * 3001 * 4 * 3  # read x once (at most), write x and y
    out["make_batch_us_events"] = per
    out["make_batch_bytes"] = moved
    out["make_batch_note"] = "device-event time per make_batch call (the launch plus the row copy); kernel time: rocprofv3"
    if a.kernel_only:
        print(json.dumps(out))
        return

    xb = {}
    for dtype in ("bf16", "fp32"):
        tr_a = PhaseNetTrainer(model, max_batch=B, dtype=dtype)
        batch = bank.make_batch(plans[0], model, SIGMA)
        xd, yd = batch["X"], batch["y"]
        torch.cuda.synchronize()
        it = iter(())

        def next_rows():
            nonlocal it
            r = next(it, None)
            if r is None:
                it = planner.epoch()
                r = next(it)
            return r

        def plain():
            tr_a.step(xd, yd, 1e-4, want_loss=False, inputs_unchanged=True)

        def fused():
            tr_a.step_bank(bank, next_rows(), 1e-4, SIGMA, want_loss=False)

        for _ in range(a.warmup):
            plain()
            fused()
        res = {"step_ms": [], "step_bank_ms": []}
        for _ in range(a.rounds):
            res["step_ms"].append(time_loop(plain, a.steps) * 1e3)
            res["step_bank_ms"].append(time_loop(fused, a.steps) * 1e3)
        tr_a.synchronize()
        res["step_ms_median"] = float(np.median(res["step_ms"]))
        res["step_bank_ms_median"] = float(np.median(res["step_bank_ms"]))
        res["ratio"] = res["step_bank_ms_median"] / res["step_ms_median"]
        res["note"] = ("step: the same resident batch every step (inputs_unchanged=True); step_bank: a new plan per step "
                       "(WindowPlanner on the host) generated into the trainer's buffers")
        xb[dtype] = res
        tr_a.close()
    out["train_step"] = xb

    if a.augment:  # the host path for contrast: the float64 numpy restatement of the same records, 32 windows scaled to B
        sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
        import augment_restate as R

        traces = list(w)
        t0 = time.perf_counter()
        for rec in plans[0][:32]:
            R.execute(rec, traces, bank.onsets, 3001, SIGMA, model.norm, model.labels)
        out["host_path"] = {"total_ms": (time.perf_counter() - t0) / 32 * B * 1e3,
                            "note": "tests/augment_restate.py execute (float64 numpy, one thread), 32 windows scaled to B"}
        bank.close()
        print(json.dumps(out))
        return

    # the host path for contrast: planner + numpy cut / normalise + gaussian_labels + upload
    w_flat = w.reshape(-1)
    hp = {"plan_ms": [], "cut_normalise_labels_ms": [], "upload_ms": []}
    for k in range(3):
        t0 = time.perf_counter()
        rows = next(planner.epoch())
        t1 = time.perf_counter()
        x, y = host_batch(w_flat, L, bank.onsets, rows)
        t2 = time.perf_counter()
        xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        hp["plan_ms"].append((t1 - t0) * 1e3)
        hp["cut_normalise_labels_ms"].append((t2 - t1) * 1e3)
        hp["upload_ms"].append((t3 - t2) * 1e3)
    hp = {k: float(np.median(v)) for k, v in hp.items()}
    hp["total_ms"] = sum(hp.values())
    hp["note"] = "one host thread of numpy; pageable upload of x and y"
    out["host_path"] = hp
    bank.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
