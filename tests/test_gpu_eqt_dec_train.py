"""GPU: EQTransformer's decoder training step (volpick_amd/csrc/train_eqt_dec.hip, vp_eqt_dec_train_*).

Every kernel is checked from the values it read (``tensors()``, ``weights()``) against the float64 formulas of
tests/eqt_dec_restate.py at bars counted from its roundings (that module's header: gamma_n sum|terms| with n = Cin K + 1
forward, Cout K + 1 for the input gradient -- the chosen form makes no pre-summed taps, the pair sum is its only extra
rounding -- B T_out for the weight and bias gradients, 89 for the head's logit, 11 for its input gradient, 5 u for the
sigmoid, 12 u for dLoss/dlogit).  ``gradients()`` is compared with float64 autograd of the restatement fed the device's
``decoder.in``; the bar is four times the worst per-tensor distance of the same restatement run in fp32 on the CPU (both
normalised by the tensor's max |g|), computed here.  The tests print what they measure; LOG.md records it.

Batch sizes: the network's lengths are fixed, so B in {1, 2, 3, 5} and B = 4 = max_batch.  No kernel tiles the batch in
groups; the weight gradient deals (window, 64-sample chunk) units to at most 256 workgroups per decoder, so that a workgroup
walks more than one unit from 257 units on: stage 6 and the head at B = 3, 4 and 5 (282, 376, 470 units), and at B = 11, where
a case of its own checks the weight gradients of stage 6 and the head alone (1034 units: four or five per workgroup)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import eqt_dec_restate as R
from tests import train_state_f64 as TS
from volpick_amd import EQTransformer, _lib
from volpick_amd import generate as G
from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows
from volpick_amd.train import EQT_LOSS_WEIGHTS, EQTransformerDecoderTrainer, EQTransformerLit

pytestmark = pytest.mark.gpu

T = 6000
W = EQT_LOSS_WEIGHTS
VP_ERR_INVALID, VP_ERR_UNSUPPORTED = -1, -4  # include/volpick_hip.h
FORWARD_BAR = 1e-4  # the project's forward contract between two implementations of the network (tests/test_gpu_eqt.py TOL)


def make_batch(B, seed, zero_row=False):
    """(x, y) fp32 (B, 3, 6000): peak-normalised synthetic windows; y rows detection box, P and S Gaussians (sigma 20).
    ``zero_row``: the last window has no labels at all."""
    rng = np.random.default_rng(seed)
    x = synthetic_windows(B, T, seed=seed).astype(np.float64)
    x -= x.mean(-1, keepdims=True)
    x /= np.abs(x).max((1, 2), keepdims=True)
    t = np.arange(T)
    y = np.zeros((B, 3, T))
    for b in range(B):
        p = rng.uniform(300, 3000)
        s = p + rng.uniform(200, 1200)
        y[b, 1] = np.exp(-((t - p) ** 2) / 800.0)
        y[b, 2] = np.exp(-((t - s) ** 2) / 800.0)
        y[b, 0, int(p):int(s + 1.4 * (s - p))] = 1.0
    if zero_row:
        y[-1] = 0.0
    return x.astype(np.float32), y.astype(np.float32)


def trainer(name="volpick", max_batch=8, **kw):
    return EQTransformerDecoderTrainer(EQTransformer.from_pretrained(name), max_batch=max_batch, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return all((bits(a[k]) == bits(b[k])).all() for k in a)


def stage_names(d, i):
    return f"{R.DEC_PREFIX[d]}.convs.{i}.weight", f"{R.DEC_PREFIX[d]}.convs.{i}.bias"


def worst(got, want, bar, where=None):
    """max |got - want| / bar (all elements, or those of the last axis listed in ``where``); inf for a non-finite value."""
    if where is not None:
        got, want, bar = got[..., where], want[..., where], bar[..., where]
    return TS.ratio(got, want, bar)


# ---- every kernel from the values it read ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, max_batch", [(1, 8), (2, 8), (3, 8), (5, 8), (4, 4)])
def test_every_kernel_from_the_values_it_read(B, max_batch):
    tr = trainer(max_batch=max_batch)
    x, y = make_batch(B, seed=10 + B, zero_row=B == 3)
    loss = tr.step(x, y, 0.0, W, update=False)
    t, w, g = tr.tensors(B), tr.weights(), tr.gradients()
    assert np.isfinite(loss) and t["decoder.in"].shape == (3, B, 16, 47) and t["p"].shape == (B, 3, T)
    r = {}  # worst error / bar per kernel, and the same on the named edge samples
    u = R.U
    for d in range(3):
        src = t["decoder.in"][d]
        for i in range(7):
            wn, bn = stage_names(d, i)
            a, abs_a = R.stage_forward(src, w[wn], w[bn], R.DOUT[i])
            bar = R.gamma(R.DCI[i] * R.DK[i] + 1) * abs_a
            edges = R.edge_samples(R.DOUT[i], R.DK[i])
            r["forward"] = max(r.get("forward", 0), worst(t[f"a{i}"][d], a, bar))
            r["forward edges"] = max(r.get("forward edges", 0), worst(t[f"a{i}"][d], a, bar, edges))
            src = t[f"a{i}"][d]
        hw, hb = w[R.HEAD_PREFIX[d] + ".weight"], w[R.HEAD_PREFIX[d] + ".bias"]
        z, abs_z = R.head_forward(t["a6"][d], hw, hb)
        r["head logit"] = max(r.get("head logit", 0), worst(t["logits"][d, :, 0], z, R.gamma(89) * abs_z))
        zd = t["logits"][d, :, 0]
        p64 = R.sigmoid(zd)
        r["sigmoid"] = max(r.get("sigmoid", 0), worst(t["p"][:, d], p64, 5 * u * p64 + R.FLOOR))
        gzh = R.head_gradient(t["p"][:, d], y[:, d], W[d], B * T)
        r["dloss/dlogit"] = max(r.get("dloss/dlogit", 0), worst(t["gz_head"][d, :, 0], gzh, 12 * u * np.abs(gzh) + R.FLOOR))
        hbk = R.head_backward(t["gz_head"][d, :, 0], t["a6"][d], hw)
        r["head input grad"] = max(r.get("head input grad", 0), worst(t["ga6"][d], hbk["ga6"], R.gamma(11) * hbk["abs_ga6"] + R.FLOOR))
        nw = B * T
        r["weight grad"] = max(r.get("weight grad", 0), worst(g[R.HEAD_PREFIX[d] + ".weight"], hbk["gw"], R.gamma(nw) * hbk["abs_gw"] + R.FLOOR))
        r["bias grad"] = max(r.get("bias grad", 0), worst(g[R.HEAD_PREFIX[d] + ".bias"], hbk["gb"], R.gamma(nw) * hbk["abs_gb"] + R.FLOOR))
        for i in range(6, -1, -1):
            wn, bn = stage_names(d, i)
            xin = t["decoder.in"][d] if i == 0 else t[f"a{i - 1}"][d]
            bk = R.stage_backward(xin, t[f"a{i}"][d], t[f"ga{i}"][d], w[wn], R.DOUT[i])
            # gz = ga (a > 0) is a selection: exact, zero at a == 0
            assert np.array_equal(t[f"gz{i}"][d], bk["gz"].astype(np.float32)), (d, i)
            nw = B * R.DOUT[i]
            r["weight grad"] = max(r["weight grad"], worst(g[wn], bk["gw"], R.gamma(nw) * bk["abs_gw"] + R.FLOOR))
            r["bias grad"] = max(r["bias grad"], worst(g[bn], bk["gb"], R.gamma(nw) * bk["abs_gb"] + R.FLOOR))
            if i > 0:
                bar = R.gamma(R.DCO[i] * R.DK[i] + 1) * bk["abs_ga_in"] + R.FLOOR
                edges = R.edge_samples(R.DIN[i], R.DK[i]) + ([186, 187] if R.DIN[i] == 188 else [])
                r["input grad"] = max(r.get("input grad", 0), worst(t[f"ga{i - 1}"][d], bk["ga_in"], bar))
                r["input grad edges"] = max(r.get("input grad edges", 0), worst(t[f"ga{i - 1}"][d], bk["ga_in"], bar, edges))
    print(f"B={B}: worst error / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(v <= 1 for v in r.values()), r
    assert (t["a2"][..., 373:] != 0).any() and (t["ga1"][..., 186:] != 0).any()  # the crop's samples carry values
    if B == 3:  # the window without labels still has gradients (p - 0), and they are finite
        assert np.isfinite(t["gz_head"]).all() and (t["gz_head"][:, 2] != 0).any()
    tr.close()


def test_weight_gradient_when_a_workgroup_walks_several_units():
    """B = 11: 94 chunks x 11 windows = 1034 units for 256 workgroups at stage 6 and at the head (module docstring)."""
    B = 11
    tr = trainer(max_batch=B)
    x, y = make_batch(B, seed=17)
    tr.step(x, y, 0.0, W, update=False)
    t, w, g = tr.tensors(B), tr.weights(), tr.gradients()
    r = np.zeros(2)
    for d in range(3):
        hbk = R.head_backward(t["gz_head"][d, :, 0], t["a6"][d], w[R.HEAD_PREFIX[d] + ".weight"])
        wn, bn = stage_names(d, 6)
        bk = R.stage_backward(t["a5"][d], t["a6"][d], t["ga6"][d], w[wn], T)
        for gw, gb, ref in ((g[R.HEAD_PREFIX[d] + ".weight"], g[R.HEAD_PREFIX[d] + ".bias"], hbk), (g[wn], g[bn], bk)):
            r = np.maximum(r, [worst(gw, ref["gw"], R.gamma(B * T) * ref["abs_gw"] + R.FLOOR),
                               worst(gb, ref["gb"], R.gamma(B * T) * ref["abs_gb"] + R.FLOOR)])
    print(f"B={B}: worst error / bar: weight grad {r[0]:.3g}, bias grad {r[1]:.3g}")
    assert (r <= 1).all(), r
    tr.close()


# ---- end to end against autograd ---------------------------------------------------------------------------------------------
def distances(grads, ref):
    return {k: float(np.abs(np.asarray(grads[k], np.float64) - ref[k]).max() / np.abs(ref[k]).max()) for k in ref}


@pytest.mark.parametrize("name, B", [("volpick", 2), ("volpick_95train", 3)])
def test_gradients_against_float64_autograd(name, B):
    tr = trainer(name)
    x, y = make_batch(B, seed=20 + B, zero_row=True)
    loss = tr.step(x, y, 0.0, W, update=False)
    dec_in, w = tr.tensors(B)["decoder.in"], tr.weights()
    loss64, g64 = R.loss_and_grads(w, dec_in, y, W, torch.float64)
    loss32, g32 = R.loss_and_grads(w, dec_in, y, W, torch.float32)
    dev, cpu = distances(tr.gradients(), g64), distances(g32, g64)
    bar = 4 * max(cpu.values())
    k_dev, k_cpu = max(dev, key=dev.get), max(cpu, key=cpu.get)
    print(f"{name} B={B}: loss {loss:.9g} (float64 {loss64:.9g}); worst distance / max|g|: device {dev[k_dev]:.3g} ({k_dev}), "
          f"fp32 CPU {cpu[k_cpu]:.3g} ({k_cpu}); bar {bar:.3g}")
    assert len(dev) == 48 and all(np.abs(g64[k]).max() > 0 for k in g64)
    assert abs(loss - loss64) <= 1e-6 * abs(loss64)  # float64 reduction of fp32 predictions
    assert max(dev.values()) <= bar, (dev[k_dev], k_dev, bar)
    tr.close()


# ---- Adam, update = 0, write_weights, set_hyper ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", [(0.9, 0.999, 1e-8), (0.5, 0.9, 1e-3)])
def test_adam_follows_float64_from_the_values_each_step_read(hyper):
    tr = trainer(betas=hyper[:2], eps=hyper[2])
    x, y = make_batch(2, seed=31)
    w0 = tr.weights()
    m0, v0 = tr.adam_state()
    assert not any(m0[k].any() or v0[k].any() for k in m0)
    # update = 0 leaves weights, moments and the count alone (and still computes gradients)
    tr.step(x, y, 1e-3, W, update=False)
    assert same_bits(tr.weights(), w0) and same_bits(tr.adam_state()[0], m0) and tr.global_step == 0
    assert any(g.any() for g in tr.gradients().values())
    worst_r = np.zeros(3)
    for t, lr in enumerate((1e-3, 3e-4, 1e-2), start=1):
        w, (m, v) = tr.weights(), tr.adam_state()
        tr.step(x, y, lr, W, update=True)
        g, w1, (m1, v1) = tr.gradients(), tr.weights(), tr.adam_state()
        for k in w:
            ref = TS.adam_update(w[k], g[k], m[k], v[k], t, lr, *hyper)
            worst_r = np.maximum(worst_r, [TS.ratio(m1[k], ref.m, ref.bar_m), TS.ratio(v1[k], ref.v, ref.bar_v),
                                           TS.ratio(w1[k], ref.w, ref.bar_w)])
        if t == 1:  # an update-free step in between does not advance the count: the next update is t = 2
            tr.step(x, y, 1.0, W, update=False)
            assert same_bits(tr.weights(), w1)
    print(f"hyper {hyper}: worst error / bar: m {worst_r[0]:.3g}, v {worst_r[1]:.3g}, w {worst_r[2]:.3g}")
    assert (worst_r <= 1).all(), worst_r
    # write_weights: the moments and the count stay; the next step computes what a new trainer computes from that blob
    blob = np.concatenate([w0[k].ravel() for k, _ in tr.names])
    m, v = tr.adam_state()
    tr.write_weights(blob)
    assert same_bits(tr.weights(), w0) and same_bits(tr.adam_state()[0], m) and same_bits(tr.adam_state()[1], v)
    loss = tr.step(x, y, 1e-3, W, update=False)
    fresh = trainer()
    assert fresh.step(x, y, 1e-3, W, update=False) == loss and same_bits(fresh.gradients(), tr.gradients())
    with pytest.raises(ValueError, match="flat blob of 145731"):
        tr.write_weights(blob[:-1])
    fresh.close(), tr.close()


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    tr = trainer(max_batch=4)
    x, y = make_batch(2, seed=33)
    tr.step(x, y, 0.0, W, update=False)
    w0, g0 = tr.weights(), tr.gradients()
    for b1, b2, eps in [(1.0, 0.999, 1e-8), (-0.1, 0.9, 1e-8), (0.9, 1.0, 1e-8), (0.9, float("nan"), 1e-8), (0.9, 0.999, 0.0),
                        (0.9, 0.999, float("inf")), (0.9, 0.999, float("nan"))]:
        assert lib.vp_eqt_dec_train_set_hyper(tr._h, b1, b2, eps) == VP_ERR_INVALID, (b1, b2, eps)
    xb, yb = make_batch(5, seed=34)
    for call, text in [(lambda: tr.step(xb, yb, 1e-3, W), "batch 5 outside"),
                       (lambda: tr.step(x, y, float("nan"), W), "learning rate"),
                       (lambda: tr.step(x, y, float("inf"), W), "learning rate"),
                       (lambda: tr.step(x, y, 1e-3, (0.05, float("nan"), 0.55)), "loss weights"),
                       (lambda: tr.step(x, y, 1e-3, (float("inf"), 0.4, 0.55)), "loss weights")]:
        with pytest.raises(_lib.VolpickHipError, match=text):
            call()
    loss = C.c_double()
    wd = (C.c_double * 3)(*W)
    assert lib.vp_eqt_dec_train_step(tr._h, _lib.ptr(x), _lib.ptr(y), _lib.VP_MEM_HOST, 0, wd, 1e-3, 1, C.byref(loss)) == VP_ERR_INVALID
    assert tr.global_step == 0 and same_bits(tr.weights(), w0) and same_bits(tr.gradients(), g0)  # nothing ran
    # a PhaseNet blob
    n = lib.vp_weight_count(_lib.VP_MODEL_PHASENET)
    h = C.c_void_p()
    rc = lib.vp_eqt_dec_train_create(0, _lib.ptr(np.zeros(n, np.float32)), n, None, 4, C.byref(h))
    assert rc == VP_ERR_UNSUPPORTED and b"PhaseNet" in lib.vp_last_error() and not h.value
    assert lib.vp_eqt_dec_train_create(0, _lib.ptr(np.zeros(10, np.float32)), 10, None, 4, C.byref(h)) == VP_ERR_INVALID
    tr.close()


# ---- bit reproducibility, export ----------------------------------------------------------------------------------------------
def test_two_trainers_hold_the_same_bits_and_export_leaves_the_trunk_alone():
    a, b = trainer(), trainer()
    batches = [make_batch(B, seed=40 + i, zero_row=i == 2) for i, B in enumerate((2, 5, 1, 3, 2))]
    for tr in (a, b):
        tr.losses = [tr.step(x, y, 1e-3, W) for x, y in batches]
    assert a.losses == b.losses and same_bits(a.weights(), b.weights()) and same_bits(a.gradients(), b.gradients())
    assert all(same_bits(s, t) for s, t in zip(a.adam_state(), b.adam_state()))
    assert a.launch_count() == b.launch_count() > 30
    before = a.model.state_dict()
    start = EQTransformer.from_pretrained("volpick").state_dict()
    model = a.export()
    after, trained = model.state_dict(), a.weights()
    assert list(after) == list(before)
    for k in after:
        if R.is_decoder_key(k):
            assert (bits(after[k]) == bits(trained[k])).all() and not (bits(after[k]) == bits(start[k])).all(), k
        else:
            assert np.array_equal(after[k], start[k]) and after[k].dtype == start[k].dtype, k
    # the exported model predicts what the trainer predicts from the same weights
    x, y = batches[0]
    a.step(x, y, 0.0, W, update=False)
    p = a.tensors(2)["p"]
    q = torch.stack(model.cuda()(torch.from_numpy(x).cuda()), 1).cpu().numpy()
    print(f"max |model(X) - trainer's predictions| = {np.abs(p - q).max():.3g}")
    assert np.abs(p - q).max() <= FORWARD_BAR
    a.close(), b.close()


# ---- it trains ---------------------------------------------------------------------------------------------------------------
def wavelet_batch(B=4, seed=50):
    """Decaying P and S wavelets on weak noise, labels from the onsets."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    x = 0.02 * rng.standard_normal((B, 3, T))
    y = np.zeros((B, 3, T))
    for b in range(B):
        p, s = rng.uniform(800, 2500), 0.0
        s = p + rng.uniform(400, 1500)
        for onset, f, amp in ((p, 0.09, 0.6), (s, 0.04, 1.0)):
            env = np.where(t >= onset, np.exp(-(t - onset) / 300.0), 0.0)
            for c in range(3):
                x[b, c] += amp * rng.uniform(0.5, 1.0) * env * np.sin(2 * np.pi * f * (t - onset) + rng.uniform(0, 6.28))
        y[b, 1] = np.exp(-((t - p) ** 2) / 800.0)
        y[b, 2] = np.exp(-((t - s) ** 2) / 800.0)
        y[b, 0, int(p):int(s + 1.4 * (s - p))] = 1.0
    x -= x.mean(-1, keepdims=True)
    x /= np.abs(x).max((1, 2), keepdims=True)
    return x.astype(np.float32), y.astype(np.float32)


def test_twelve_steps_lower_the_loss_as_the_float64_oracle_does():
    tr = trainer()
    x, y = wavelet_batch()
    first = tr.step(x, y, 0.0, W, update=False)
    dec_in = tr.tensors(4)["decoder.in"]  # the trunk is frozen: the same tensor in every step
    oracle, _ = R.adam_train(tr.weights(), dec_in, y, W, 1e-3, 12)
    assert oracle[11] < 0.95 * oracle[0], oracle  # the precondition: this batch can be learnt from
    losses = [tr.step(x, y, 1e-3, W) for _ in range(12)]
    ratio, want = losses[11] / losses[0], oracle[11] / oracle[0]
    print(f"loss {losses[0]:.6g} -> {losses[11]:.6g} (ratio {ratio:.4f}); float64 oracle {oracle[0]:.6g} -> {oracle[11]:.6g} ({want:.4f})")
    assert losses[0] == first and abs(losses[0] - oracle[0]) <= 1e-6 * oracle[0]
    assert abs(ratio - want) <= 0.01
    tr.close()


# ---- generated batches, fit_bank, the lit ----------------------------------------------------------------------------------------
def eqt_bank(n=24, seed=61):
    rng = np.random.default_rng(seed)
    traces, ps, ss = [], [], []
    for i, L in enumerate(np.linspace(7000, 14000, n).astype(int)):
        x, p, s = synthetic_stream_array(int(L), seed=seed * 100003 + i, n_events=1)
        traces.append(np.ascontiguousarray(x * rng.uniform(0.1, 100.0), np.float32))
        ps.append(float(p[0]))
        ss.append(float(s[0]) if i % 5 else np.nan)
    return G.WaveformBank(traces, {"P": ps, "S": ss})


@pytest.fixture(scope="module")
def bank():
    b = eqt_bank()
    yield b
    b.close()


def augmentation(bank):
    n = bank.n_traces
    return G.Augmentation(event_traces=np.arange(4, n), noise_traces=np.arange(0, 4), val_event_traces=np.arange(4, n),
                          val_noise_traces=np.arange(0, 4))


@pytest.mark.parametrize("kind", ["plan rows", "augmented rows"])
def test_step_bank_equals_make_batch_and_step(bank, kind):
    a, b = trainer(), trainer()
    lit = EQTransformerLit(model=a.model, sigma=20, detection_fixed_window=None)
    pick = np.random.default_rng(7).integers(0, bank.n_traces, 5)
    if kind == "plan rows":
        rows = lit.window_planner(bank, 5, seed=3).plan(pick)
    else:
        rows = lit.augmented_planner(bank, 5, augmentation(bank), seed=3).plan(pick)
        assert rows.dtype == G.AUG_ROW
    made = lit.make_batch(bank, rows)
    y3 = torch.cat([made["detections"], made["y"]], 1)
    la = a.step_bank(bank, rows, 1e-3, 20, W)
    lb = b.step(made["X"], y3, 1e-3, W)
    assert la == lb and np.isfinite(la)
    assert same_bits(a.gradients(), b.gradients()) and same_bits(a.weights(), b.weights())
    assert (bits(a.tensors(5)["p"]) == bits(b.tensors(5)["p"])).all()
    with pytest.raises(_lib.VolpickHipError, match="outside"):
        a.step_bank(bank, np.concatenate([rows, rows]), 1e-3, 20, W)  # 10 > max_batch 8
    a.close(), b.close()


def test_fit_bank_steps_the_scheduler_and_keeps_the_best_decoders(bank):
    lit = EQTransformerLit(lr=1e-2, sigma=20, model=EQTransformer.from_pretrained("volpick"), trainable="decoders", max_batch=8)
    n = bank.n_traces
    train = G.WaveformBank([bank.trace(i) for i in range(16)], {"P": bank.onsets[:16, :2], "S": bank.onsets[:16, 2:]})
    val = G.WaveformBank([bank.trace(i) for i in range(16, n)], {"P": bank.onsets[16:, :2], "S": bank.onsets[16:, 2:]})
    try:
        losses, val_losses = lit.fit_bank(train, 4, batch_size=8, seed=1, val_bank=val, lr_scheduler="ReduceLROnPlateau",
                                          lr_scheduler_args={"factor": 0.5, "patience": 0, "threshold": 0.5}, keep_best=True)
        assert len(losses) == 4 and len(val_losses) == 2 and np.isfinite(losses).all() and np.isfinite(val_losses).all()
        h = lit.history
        assert h["val_loss"] == val_losses and len(h["lr"]) == 2 and h["best"][2] == min(val_losses)
        # the scheduler was stepped: with this threshold the second validation cannot count as better, so the rate it leaves
        # is half the one it was given (the warm-up's lr * 4 / 500)
        assert h["lr"][1] == pytest.approx(0.5 * lit.lr * 4 / 500)
        tr = lit.trainer_state
        assert tr.global_step == 4 and set(lit.best_state) == {k for k, _ in tr.names}
        assert same_bits(tr.weights(), lit.best_state)  # keep_best restored the best decoders into the trainer ...
        sd = lit.model.state_dict()
        assert all((bits(sd[k]) == bits(lit.best_state[k])).all() for k in lit.best_state)  # ... and the model
        assert np.isfinite(lit.validate_bank(val, lit.window_planner(val, 8, seed=2))).all()  # the restored model validates
    finally:
        train.close(), val.close()
        lit.trainer_state.close()


def test_the_lit_trains_with_trainable_decoders(bank):
    """Fails without the feature: ``training_step`` raised NotImplementedError for every EQTransformerLit."""
    lit = EQTransformerLit(lr=1e-3, model=EQTransformer.from_pretrained("volpick"), trainable="decoders", max_batch=8)
    rows = lit.window_planner(bank, 4, seed=5).plan(np.arange(4))
    batch = lit.make_batch(bank, rows)
    w0 = {k: v.copy() for k, v in lit.trainer_state.weights().items()}
    loss = lit.training_step(batch)
    w1 = lit.trainer_state.weights()
    assert np.isfinite(loss) and loss > 0 and lit.trainer_state.global_step == 1
    assert all((bits(w0[k]) != bits(w1[k])).any() for k in w0)
    # the validation path sees the trained weights: the same batch scores differently after the step
    host = lit.validation_step(batch)
    untrained = EQTransformerLit(model=EQTransformer.from_pretrained("volpick")).validation_step(batch)
    # (the step's loss is that of the weights before the update: the untrained model's, up to the forward paths' difference)
    assert abs(untrained - loss) <= 1e-2 * loss and host != untrained
    with pytest.raises(NotImplementedError):
        EQTransformerLit(model=lit.model).training_step(batch)
    lit.trainer_state.close()
