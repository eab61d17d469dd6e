#!/usr/bin/env python3
"""What one validation batch costs beside one training step (LOG.md), on a synthetic bank.

At B = 512 and B = 64, medians after warm-up:
  host    ms per batch of ``PhaseNetLit.validation_step(bank.make_batch(rows))``: forward on the GPU, predictions and
          labels copied back, float64 numpy loss on one host thread (each batch ends with the host holding its loss);
  device  ms per batch of ``validate_batches``: passes of N batches between one vp_validate_begin and vp_validate_end
          (pass time / N), and the latency of a pass of one batch;
  stages  of the device batch, each alone between HIP events: generation, forward, loss kernel;
  export  ms of one ``PhaseNetTrainer.export()`` and of the handle rebuild (``model.cuda()``) that follows it;
  step    ms of one ``step_bank`` as ``fit_bank`` runs it (the loss read back every step) and with the steps queued.
``--model eqtransformer`` times EQTransformer's pass instead (``validate_batches_eqt``, B = 256 and B = 64): the device
batch, generation, forward and the weighted-BCE kernel each alone, the host route of ``EQTransformerLit.validation_step``,
and ``vp_vce_loss`` on the loss kernel's arrays -- the same bytes with one float64 logarithm per element instead of two;
then the stacked recipe beside block 1 (``aug_*``: ``EQTransformerLit.augmented_planner`` with the reference's branch
probabilities, ``vp_bank_make_batch_eqt_aug`` / ``vp_validate_eqt_bank_aug``), the two alternating call by call: generation
alone as one call between two events and as 20 calls queued between two events (the row upload of a call then runs under
the previous call's kernel), and the device batch in a pass.
usage: validate_timing.py [--batches 20] [--passes 7] [--model phasenet|eqtransformer]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from volpick_amd import PhaseNet, _lib  # noqa: E402
from volpick_amd import generate as G  # noqa: E402
from volpick_amd.synthetic import synthetic_stream_array  # noqa: E402
from volpick_amd.train import PhaseNetLit, validate_batches, vector_cross_entropy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=20, help="batches per device pass, and host batches / steps timed")
ap.add_argument("--passes", type=int, default=7)
ap.add_argument("--traces", type=int, default=128)
ap.add_argument("--model", choices=("phasenet", "eqtransformer"), default="phasenet")
args = ap.parse_args()
N = max(20, args.batches)


def wall_ms(fn, n, warm=3):
    """Median wall time of fn() in ms over n calls after `warm` calls; the GPU is idle at the start of each."""
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def event_ms(fn, n, warm=3):
    """Median time of what fn() enqueues on torch's current stream, between two events."""
    out = []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return float(np.median(out))


def alternating_ms(fa, fb, n, warm=2, timer=None):
    """Medians of fa() and fb() timed turn by turn (a, b, a, b, ...), so that both see the same machine."""
    timer = timer or wall_ms
    a, b = [], []
    for i in range(warm + n):
        ta, tb = timer(fa, 1, warm=0), timer(fb, 1, warm=0)
        if i >= warm:
            a.append(ta)
            b.append(tb)
    return float(np.median(a)), float(np.median(b))


rng = np.random.default_rng(0)
xs, ps, ss = [], [], []
for i in range(args.traces):
    x, p, s = synthetic_stream_array(20000 if args.model == "eqtransformer" else 9000, seed=1000 + i, n_events=1)
    xs.append(x * rng.uniform(0.1, 100.0))
    ps.append(float(p[0]))
    ss.append(float(s[0]))
bank = G.WaveformBank(np.stack(xs).astype(np.float32), {"P": ps, "S": ss})
lib = _lib.load()
result = {}


def eqtransformer_mode():
    """--model eqtransformer: the device batch in a pass, its stages alone and the host route, at B = 256 and B = 64; and the
    loss kernel beside vp_vce_loss on the same arrays (the same bytes, one float64 logarithm per element instead of two)."""
    from volpick_amd import EQTransformer
    from volpick_amd.train import EQTransformerLit, bce_loss, validate_batches_eqt

    for B in (256, 64):
        lit = EQTransformerLit(model=EQTransformer.from_pretrained("volpick").cuda())
        model = lit.model
        planner = lit.window_planner(bank, B, seed=B)
        plans = [planner.plan(rng.integers(0, args.traces, B)) for _ in range(N)]
        r = result[f"B{B}"] = {}
        it = iter(plans * 4)
        r["host_ms_per_batch"] = wall_ms(lambda: lit.validation_step(lit.make_batch(bank, next(it))), N)
        r["device_ms_per_batch_in_a_pass"] = wall_ms(lambda: validate_batches_eqt(model, bank, plans, lit.sigma), args.passes, warm=2) / N
        it = iter(plans * 4)
        r["device_ms_single_batch_pass"] = wall_ms(lambda: validate_batches_eqt(model, bank, [next(it)], lit.sigma), N)

        it = iter(plans * 4)
        made = lit.make_batch(bank, plans[0])
        r["stage_generate_ms"] = event_ms(lambda: lit.make_batch(bank, next(it)), N)
        r["stage_forward_ms"] = wall_ms(lambda: model(made["X"]), N)  # (vp_forward waits for its stream itself)
        pred = torch.stack(model(made["X"]), 1).contiguous()
        y = torch.cat([made["detections"], made["y"]], 1).contiguous()
        hd = torch.empty(3 * B, dtype=torch.float64, device="cuda")
        pw = torch.empty(B, dtype=torch.float64, device="cuda")
        bt = torch.empty(1, dtype=torch.float64, device="cuda")
        w = (C.c_double * 3)(*lit.loss_weights)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        r["stage_loss_kernel_ms"] = event_ms(
            lambda: _lib.check(lib.vp_bce_loss(0, ptr(pred), ptr(y), B, 3, 6000, w, ptr(hd), ptr(pw), ptr(bt), stream)), N)
        r["vce_kernel_same_arrays_ms"] = event_ms(
            lambda: _lib.check(lib.vp_vce_loss(0, ptr(pred), ptr(y), B, 3, 6000, 1e-5, ptr(pw), ptr(bt), stream)), N)
        r["loss_kernel_GB_per_s"] = 2 * 4 * pred.numel() / (1e6 * r["stage_loss_kernel_ms"])
        p_host, y_host = pred.cpu().numpy(), y.cpu().numpy()
        r["host_copy_back_ms"] = wall_ms(lambda: (pred.cpu(), y.cpu()), N)
        t0 = time.perf_counter()
        for _ in range(3):
            bce_loss(p_host, y_host, lit.loss_weights)
        r["host_numpy_loss_ms"] = 1e3 * (time.perf_counter() - t0) / 3
        # the stacked recipe beside block 1: the first three quarters of the bank as event sources, the rest as noise sources
        n_ev = 3 * args.traces // 4
        aug = G.Augmentation(val_event_traces=np.arange(n_ev), val_noise_traces=np.arange(n_ev, args.traces))
        aplanner = lit.augmented_planner(bank, B, aug, seed=B, validation=True)
        aplans = [aplanner.plan(rng.integers(0, args.traces, B)) for _ in range(N)]
        allrows = np.concatenate(aplans)
        r["aug_fraction_with_event"] = float((allrows["event"]["kind"] != 0).any(axis=1).mean())
        r["aug_fraction_with_stacked_noise"] = float((allrows["noise"]["kind"] != 0).any(axis=1).mean())
        r["aug_fraction_with_gauss"] = float((allrows["gauss"] > 0).mean())
        r["aug_fraction_with_gap"] = float((allrows["gap_hi"] > allrows["gap_lo"]).mean())
        r["aug_source_windows_per_window"] = float(((allrows["event"]["kind"] != 0).sum(axis=1)
                                                    + (allrows["noise"]["kind"] != 0).sum(axis=1)).mean())
        ia, ib = iter(plans * 40), iter(aplans * 40)
        r["generate_ms"], r["aug_generate_ms"] = alternating_ms(
            lambda: lit.make_batch(bank, next(ia)), lambda: lit.make_batch(bank, next(ib)), 4 * N, warm=5, timer=event_ms)

        def queued(batches):
            for rows in batches:
                lit.make_batch(bank, rows)

        q0, q1 = alternating_ms(lambda: queued(plans), lambda: queued(aplans), 15, warm=3, timer=event_ms)
        r["generate_ms_queued"], r["aug_generate_ms_queued"] = q0 / N, q1 / N
        p0, p1 = alternating_ms(lambda: validate_batches_eqt(model, bank, plans, lit.sigma),
                                lambda: validate_batches_eqt(model, bank, aplans, lit.sigma), max(args.passes, 9), warm=2)
        r["device_ms_per_batch_in_a_pass_again"], r["aug_device_ms_per_batch_in_a_pass"] = p0 / N, p1 / N
        print(f"B = {B}")
        for k, v in r.items():
            print(f"  {k:38s} {v:9.3f}")


if args.model == "eqtransformer":
    eqtransformer_mode()
    bank.close()
    print(json.dumps({"validate_timing_eqtransformer": result}))
    sys.exit(0)

for B in (512, 64):
    lit = PhaseNetLit(lr=1e-3, model=PhaseNet.from_pretrained("volpick"), max_batch=B)
    tr = lit._ensure()
    planner = G.WindowPlanner(bank, B, seed=B)
    plans = [planner.plan(rng.integers(0, args.traces, B)) for _ in range(N)]
    model = lit._exported_model()
    r = result[f"B{B}"] = {}

    it = iter(plans * 4)
    r["host_ms_per_batch"] = wall_ms(lambda: lit.validation_step(bank.make_batch(next(it), model, lit.sigma)), N)
    r["device_ms_per_batch_in_a_pass"] = wall_ms(lambda: validate_batches(model, bank, plans, lit.sigma), args.passes, warm=2) / N
    it = iter(plans * 4)
    r["device_ms_single_batch_pass"] = wall_ms(lambda: validate_batches(model, bank, [next(it)], lit.sigma), N)

    # the stages of a device batch, each alone
    it = iter(plans * 4)
    made = bank.make_batch(plans[0], model, lit.sigma)
    r["stage_generate_ms"] = event_ms(lambda: bank.make_batch(next(it), model, lit.sigma), N)
    r["stage_forward_ms"] = wall_ms(lambda: model(made["X"]), N)  # (vp_forward waits for its stream itself)
    pred = model(made["X"])
    pw = torch.empty(B, dtype=torch.float64, device="cuda")
    bt = torch.empty(1, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r["stage_loss_kernel_ms"] = event_ms(
        lambda: _lib.check(lib.vp_vce_loss(0, C.c_void_p(pred.data_ptr()), C.c_void_p(made["y"].data_ptr()), B, 3, 3001, 1e-5,
                                           C.c_void_p(pw.data_ptr()), C.c_void_p(bt.data_ptr()), stream)), N)
    # the host path's own parts
    p_host, y_host = pred.cpu().numpy(), made["y"].cpu().numpy()
    r["host_copy_back_ms"] = wall_ms(lambda: (pred.cpu(), made["y"].cpu()), N)
    t0 = time.perf_counter()
    for _ in range(5):
        vector_cross_entropy(p_host.astype(np.float64), y_host.astype(np.float64))
    r["host_numpy_loss_ms"] = 1e3 * (time.perf_counter() - t0) / 5

    # the stacked recipe (vp_bank_make_batch_aug, vp_train_step_bank_aug): sources as in the EQTransformer mode
    n_ev = 3 * args.traces // 4
    aug = G.Augmentation(val_event_traces=np.arange(n_ev), val_noise_traces=np.arange(n_ev, args.traces))
    aplanner = aug.planner(bank, B, seed=B, sigma=lit.sigma, validation=True)
    aplans = [aplanner.plan(rng.integers(0, args.traces, B)) for _ in range(N)]
    ib = iter(aplans * 40)
    r["aug_generate_ms"] = event_ms(lambda: bank.make_batch(next(ib), model, lit.sigma), 4 * N, warm=5)
    r["aug_generate_ms_queued"] = event_ms(lambda: [bank.make_batch(rows, model, lit.sigma) for rows in aplans], 15) / N
    ib = iter(aplans * 4)
    r["aug_train_step_ms_fp32"] = wall_ms(lambda: tr.step_bank(bank, next(ib), 1e-3, lit.sigma), N)

    for prec in ("32", "bf16-mixed"):
        lt = lit if prec == "32" else PhaseNetLit(lr=1e-3, model=PhaseNet.from_pretrained("volpick"), max_batch=B, precision=prec)
        t = lt._ensure()
        it = iter(plans * 4)
        key = "fp32" if prec == "32" else "bf16"
        r[f"train_step_ms_{key}"] = wall_ms(lambda: t.step_bank(bank, next(it), 1e-3, lt.sigma), N)

        def queued():
            for rows in plans:
                t.step_bank(bank, rows, 1e-3, lt.sigma, want_loss=False)
            t.synchronize()

        r[f"train_step_ms_{key}_queued"] = wall_ms(queued, 3, warm=1) / N

    r["export_ms"] = wall_ms(lambda: tr.export(), 5, warm=1)

    def export_and_rebuild():
        tr.export()
        lit.model.cuda(0)

    r["export_and_handle_rebuild_ms"] = wall_ms(export_and_rebuild, 5, warm=1)
    print(f"B = {B}")
    for k, v in r.items():
        print(f"  {k:34s} {v:9.3f} ms")
    r["device_batch_below_train_step"] = bool(r["device_ms_per_batch_in_a_pass"] < r["train_step_ms_fp32"])
bank.close()
print(json.dumps({"validate_timing": result}))
