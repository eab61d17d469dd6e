"""GPU: the validation loss on the device.  The float64 cross-entropy kernel (csrc/valloss.hip, vp_vce_loss) against the
numpy float64 oracle at a-priori bars (tests/valloss_f64.py); one validation batch from a bank on a picker handle
(vp_validate_begin / _bank / _end) against the oracle on the predictions it returns; ``PhaseNetLit.validate_bank`` against
the host path; and ``fit_bank`` with device validation, the LR-on-plateau schedule, the best weights and the early stop."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import valloss_f64 as V
from tests.test_gpu_generate import synthetic_bank
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd import generate as G
from volpick_amd.train import PhaseNetLit, validate_batches

pytestmark = pytest.mark.gpu

T = 3001
SENTINEL = -12345.0


def vce(p, y, eps=1e-5, per_window=True, batch=True, shape=None):
    """vp_vce_loss on CUDA tensors: (return code, per-window values or None, batch value or None)."""
    lib = _lib.load()
    B, Cc, Tt = shape or p.shape
    pw = torch.full((max(B, 1),), SENTINEL, dtype=torch.float64, device="cuda") if per_window else None
    bt = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda") if batch else None
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.vp_vce_loss(0, C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), B, Cc, Tt, eps,
                         C.c_void_p(pw.data_ptr()) if per_window else None, C.c_void_p(bt.data_ptr()) if batch else None,
                         C.c_void_p(stream))
    torch.cuda.synchronize()
    return rc, (pw.cpu().numpy() if per_window else None), (float(bt.cpu()[0]) if batch else None)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


SHAPES = [(1, 3, 3001), (2, 3, 3001), (5, 3, 3001), (3, 1, 7), (2, 3, 6000), (257, 3, 3001)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_is_within_the_bars_of_the_float64_oracle(shape):
    """Every input kind at every shape: window values and the batch value inside the a-priori bars, a second launch equal
    to the bit, and either output left out (the batch value alone has the same bits as beside the window values)."""
    for kind in V.INPUT_KINDS:
        p, y = V.make_inputs(kind, shape, seed=len(kind) + shape[0])
        pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
        rc, pw, bt = vce(pd, yd)
        assert rc == 0, _lib.last_error()
        want, bar = V.per_window_loss(p, y), V.bar(p, y)
        err = np.abs(pw - want)
        print(f"{kind} {shape}: max window err / bar = {(err / np.maximum(bar, 1e-300)).max():.3g}, "
              f"batch err / bar = {abs(bt - want.mean()) / max(V.batch_bar(p, y), 1e-300):.3g}")
        assert (err <= bar).all(), (kind, err.max(), bar.min())
        assert abs(bt - want.mean()) <= V.batch_bar(p, y), (kind, bt, want.mean())
        if kind == "y_zero":
            assert (pw == 0).all() and bt == 0
        if kind == "p_zero_stretch":  # a float eps widened to double would miss the bar: each such term moves by 2.5e-8 |y|
            moved = np.abs(V.per_window_loss(p, y, eps=float(np.float32(1e-5))) - want)
            assert (moved > 50 * bar).all()
        rc2, pw2, bt2 = vce(pd, yd)
        assert rc2 == 0 and (bits(pw2) == bits(pw)).all() and bits(bt2) == bits(bt)
        rc3, pw3, none = vce(pd, yd, batch=False)
        assert rc3 == 0 and none is None and (bits(pw3) == bits(pw)).all()
        if shape[0] <= 5:  # (one workgroup walks the windows: not the path for large batches)
            rc4, none, bt4 = vce(pd, yd, per_window=False)
            assert rc4 == 0 and none is None and bits(bt4) == bits(bt)


def test_kernel_reads_p_and_y_of_different_alignment():
    """y four bytes further than p from a 16-byte boundary: no wide loads, the same bars."""
    p, y = V.make_inputs("softmax", (3, 3, 3001), seed=9)
    pd = torch.from_numpy(p).cuda()
    ybuf = torch.empty(y.size + 1, dtype=torch.float32, device="cuda")
    ybuf[1:] = torch.from_numpy(y.ravel()).cuda()
    rc, pw, bt = vce(pd, ybuf[1:], shape=(3, 3, 3001))
    assert rc == 0, _lib.last_error()
    want = V.per_window_loss(p, y)
    assert (np.abs(pw - want) <= V.bar(p, y)).all() and abs(bt - want.mean()) <= V.batch_bar(p, y)


def test_kernel_propagates_non_finite_values():
    p, y = V.make_inputs("softmax", (5, 3, 3001), seed=4)
    p[1, 2, 1234] = np.nan
    p[3, 0, 7] = np.inf
    y[3, 0, 7] = 0.5
    rc, pw, bt = vce(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())
    assert rc == 0
    want, bar = V.per_window_loss(p, y), V.bar(p, y)
    assert np.isnan(pw[1]) and np.isnan(want[1]) and np.isnan(bt)
    assert pw[3] == want[3] == -np.inf
    ok = [0, 2, 4]
    assert (np.abs(pw[ok] - want[ok]) <= bar[ok]).all()


@pytest.mark.parametrize("bad", [dict(B=0), dict(C=0), dict(C=9), dict(T=0), dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan"))])
def test_kernel_argument_errors_launch_nothing(bad):
    p = torch.full((2, 3, 64), 0.3, device="cuda")
    a = dict(B=2, C=3, T=64, eps=1e-5)
    a.update(bad)
    rc, pw, bt = vce(p, p, eps=a["eps"], shape=(a["B"], a["C"], a["T"]))
    assert rc == -1 and _lib.last_error()  # VP_ERR_INVALID
    assert (pw == SENTINEL).all() and bt == SENTINEL


# ---------------------------------------------------------------------------------------------------------- bank path
@pytest.fixture(scope="module")
def setup():
    _, _, _, bank = synthetic_bank(40, L=9000, seed=12)
    model = PhaseNet.from_pretrained("volpick").cuda()
    yield bank, model
    bank.close()


def planned_rows(bank, B, kind, seed):
    traces = np.random.default_rng(seed).integers(0, 40, B)
    if kind == "window":
        return G.WindowPlanner(bank, B, seed=seed).plan(traces)
    return G.AugmentedPlanner(bank, B, np.arange(0, 30), np.arange(30, 40), seed=seed, sigma=20, event_prob=(1, 1, 1),
                              noise_prob=(1, 1, 1), gap_prob=(1, 1)).plan(traces)


@pytest.mark.parametrize("kind", ["window", "augmented"])
@pytest.mark.parametrize("B", [1, 5, 64, 257])
def test_one_batch_from_a_bank(setup, B, kind):
    """Window and batch losses within the bars of the oracle on the predictions handed back and the labels of
    ``make_batch``; the predictions are bit-equal to ``model(batch["X"])`` (observed difference: 0), also across the
    max_batch = 256 chunk boundary, where B = 257 leaves a chunk of one window."""
    bank, model = setup
    rows = planned_rows(bank, B, kind, seed=B)
    batch, window, preds = validate_batches(model, bank, [rows], 20, predictions=True)
    made = bank.make_batch(rows, model, 20)
    p, y = preds[0].cpu().numpy(), made["y"].cpu().numpy()
    assert batch.shape == (1,) and window.shape == (B,) and p.shape == (B, 3, T)
    want, bar = V.per_window_loss(p, y), V.bar(p, y)
    assert np.isfinite(want).all() and (want > 0).all()
    assert (np.abs(window - want) <= bar).all(), (np.abs(window - want) / bar).max()
    assert abs(batch[0] - want.mean()) <= V.batch_bar(p, y)
    direct = model(made["X"]).cpu().numpy()
    diff = np.abs(direct - p).max()
    print(f"B={B} {kind}: max|pred - model(X)| = {diff:.3g}")
    assert (direct.view(np.uint32) == p.view(np.uint32)).all(), diff


def test_a_pass_of_seven_batches_equals_seven_passes(setup):
    bank, model = setup
    sizes = [5, 64, 1, 33, 64, 7, 12]
    plans = [planned_rows(bank, B, "augmented" if i % 2 else "window", seed=50 + i) for i, B in enumerate(sizes)]
    batch, window = validate_batches(model, bank, plans, 20)
    assert batch.shape == (7,) and window.shape == (sum(sizes),)
    off = 0
    for rows, b in zip(plans, batch):
        one_b, one_w = validate_batches(model, bank, [rows], 20)
        assert bits(one_b[0]) == bits(b)
        assert (bits(one_w) == bits(window[off:off + len(rows)])).all()
        off += len(rows)
    again = validate_batches(model, bank, plans, 20)
    assert (bits(again[0]) == bits(batch)).all() and (bits(again[1]) == bits(window)).all()


def test_invalid_rows_and_arguments_enqueue_nothing(setup):
    bank, model = setup
    lib = _lib.load()
    h = model._ensure_handle()
    rows = planned_rows(bank, 4, "window", seed=1)
    lrows = G.label_rows(model.labels).ctypes.data_as(C.POINTER(C.c_int))

    def call(r, eps=1e-5):
        return lib.vp_validate_bank(h, bank.handle, r.ctypes.data_as(C.c_void_p), len(r), 20.0, G._norm(model.norm), lrows, eps,
                                    None)

    assert call(rows) == -1  # no pass is open
    assert lib.vp_validate_begin(h) == 0
    bad = rows.copy()
    bad["trace"][2] = 40
    assert call(bad) == -1 and "trace" in _lib.last_error()
    assert call(rows, eps=0.0) == -1
    assert call(rows) == 0
    nb, nw = C.c_longlong(), C.c_longlong()
    one = np.full(1, SENTINEL)
    four = np.full(8, SENTINEL)
    assert lib.vp_validate_end(h, one.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(nb),
                               four.ctypes.data_as(C.POINTER(C.c_double)), 8, C.byref(nw)) == 0
    assert (nb.value, nw.value) == (1, 4)  # the refused calls left nothing behind
    assert one[0] != SENTINEL and (four[:4] != SENTINEL).all() and (four[4:] == SENTINEL).all()
    assert bits(one[0]) == bits(validate_batches(model, bank, [rows], 20)[0][0])


def test_an_eqtransformer_handle_is_unsupported(setup):
    bank, _ = setup
    lib = _lib.load()
    eqt = EQTransformer.from_pretrained("volpick").cuda()
    h = eqt._ensure_handle()
    assert lib.vp_validate_begin(h) == -4 and "PhaseNet" in _lib.last_error()  # VP_ERR_UNSUPPORTED
    rows = planned_rows(bank, 2, "window", seed=1)
    lrows = G.label_rows("PSN").ctypes.data_as(C.POINTER(C.c_int))
    assert lib.vp_validate_bank(h, bank.handle, rows.ctypes.data_as(C.c_void_p), 2, 20.0, 0, lrows, 1e-5, None) == -4


def host_batches(lit, val, planner):
    """The host path batch by batch: (loss, p, y) as ``validation_step`` sees them."""
    out = []
    for rows in planner.validation():
        b = val.make_batch(rows, lit.model, lit.sigma)
        loss = lit.validation_step(b)
        out.append((loss, lit.model(b["X"]).cpu().numpy(), b["y"].cpu().numpy()))
    return out


def test_validate_bank_equals_the_host_path(setup):
    """Batch by batch within twice the batch bar: the device's rounding and the host's own float64 rounding."""
    val, _ = setup
    lit = PhaseNetLit(model=PhaseNet.from_pretrained("volpick"), max_batch=16)
    got, window = lit.validate_bank(val, G.WindowPlanner(val, 16, seed=3), per_window=True)
    host = host_batches(lit, val, G.WindowPlanner(val, 16, seed=3))
    assert len(got) == len(host) == 3 and window.shape == (40,)  # 16 + 16 + 8: the partial batch is kept
    for g, (loss, p, y) in zip(got, host):
        assert abs(g - loss) <= 2 * V.batch_bar(p, y), (g, loss)
    rows = G.WindowPlanner(val, 16, seed=3).plan(np.arange(16))  # one array of rows is one batch: the pass's first
    one = lit.validate_bank(val, rows)
    assert len(one) == 1 and bits(one[0]) == bits(got[0]) and bits(lit.validate_bank(val, [rows])[0]) == bits(got[0])
    want = np.concatenate([V.per_window_loss(p, y) for _, p, y in host])
    assert (np.abs(window - want) <= np.concatenate([V.bar(p, y) for _, p, y in host])).all()


# ---------------------------------------------------------------------------------------------------------------- fit
@pytest.fixture(scope="module")
def fit_setup():
    """The banks and the random initialisation of test_gpu_generate.py::test_fit_bank_learns_from_a_random_initialisation."""
    from oracle.models import PhaseNet as TorchPhaseNet

    torch.manual_seed(2)
    state = {k: v.detach().numpy() for k, v in TorchPhaseNet(phases="PSN", norm="peak").state_dict().items()}
    _, _, _, bank = synthetic_bank(256, L=9000, seed=11)
    _, _, _, val = synthetic_bank(40, L=9000, seed=12)

    def new_lit(**kw):
        model = PhaseNet(phases="PSN", norm="peak")
        model.load_state_dict(state)
        return PhaseNetLit(lr=1e-2, model=model, max_batch=64, precision="bf16-mixed", **kw)

    yield bank, val, new_lit
    bank.close()
    val.close()


def test_fit_with_device_validation_equals_the_fit_with_host_validation(fit_setup):
    bank, val, new_lit = fit_setup
    host, dev = new_lit(), new_lit()
    losses_h, val_h = host.fit_bank(bank, 50, batch_size=64, seed=0, val_bank=val)
    losses_d, val_d = dev.fit_bank(bank, 50, batch_size=64, seed=0, val_bank=val, validation="device")
    assert losses_h == losses_d and len(losses_h) == 50
    assert len(val_h) == len(val_d) == 13 and np.isfinite(val_d).all()
    # One batch of 40 windows per validation.  Every term y log(p + eps) of a softmax output is <= 0 (but for p within 1e-5
    # of 1), so sum|terms| / T is the loss itself and the batch bar is (2 C T + 2 B) 2^-53 L -- from the smaller of the two
    # losses, never wider than the bar of the p and y behind them -- and twice that for the host's own rounding.
    bar = 2 * (2 * 3 * T + 2 * 40) * V.U * np.minimum(val_h, val_d)
    print("max |host - device| / bar", (np.abs(np.array(val_h) - val_d) / bar).max())
    assert (np.abs(np.array(val_h) - val_d) <= bar).all()
    assert host.history["val_loss"] == val_h and host.history["lr"] == [host.learning_rate(s) for s in range(4, 52, 4)] + [host.learning_rate(50)]


def test_fit_with_the_plateau_schedule_keeps_the_best_weights(fit_setup):
    bank, val, new_lit = fit_setup
    lit = new_lit()
    lit.WARMUP_STEPS = 8
    args = {"factor": 0.5, "patience": 0, "min_lr": 1e-6}
    losses, val_losses = lit.fit_bank(bank, 26, batch_size=64, seed=0, val_bank=val, validation="device",
                                      lr_scheduler="ReduceLROnPlateau", lr_scheduler_args=args, keep_best=True)
    assert len(losses) == 26 and len(val_losses) == 7 and np.isfinite(val_losses).all()
    used, after = V.torch_warmup_plateau(1e-2, 8, 26, 4, val_losses, **args)
    assert lit.history["lr"] == after and lit.history["val_loss"] == val_losses
    i = int(np.argmin(val_losses))  # (argmin: the first one on a tie)
    assert lit.history["best"] == (i, min(4 * (i + 1), 26), val_losses[i]) and not lit.history["stopped_early"]
    # the snapshot in a fresh model, on the windows of validation i (the planner's draws replayed), gives that loss
    fresh = PhaseNet(phases="PSN", norm="peak")
    sd = lit.model.state_dict()
    sd.update(lit.best_state)
    fresh.load_state_dict(sd)
    planner = G.WindowPlanner(val, 64, seed=1)
    for _ in range(i):
        list(planner.validation())
    plans = list(planner.validation())
    batch, _, preds = validate_batches(fresh.cuda(), val, plans, lit.sigma, predictions=True)
    bar = np.mean([V.batch_bar(p.cpu().numpy(), val.make_batch(r, fresh, lit.sigma)["y"].cpu().numpy()) for p, r in zip(preds, plans)])
    assert abs(float(np.mean(batch)) - val_losses[i]) <= bar, (float(np.mean(batch)), val_losses[i])


def test_fit_stops_early_when_the_validation_loss_stalls(fit_setup, monkeypatch):
    """The loss is made to stall: from the second validation on nothing below the first is reported."""
    bank, val, new_lit = fit_setup
    lit = new_lit()
    real, floor = lit.validate_bank, []

    def stalled(val_bank, planner):
        vl = real(val_bank, planner)
        floor.append(float(np.mean(vl)))
        return [max(v, floor[0]) for v in vl]

    monkeypatch.setattr(lit, "validate_bank", stalled)
    losses, val_losses = lit.fit_bank(bank, 30, batch_size=64, seed=0, val_bank=val, validation="device", early_stop_patience=1)
    assert lit.history["stopped_early"] and len(val_losses) == 2 and len(losses) == 8
    assert lit.history["best"] == (0, 4, val_losses[0]) and val_losses[1] >= val_losses[0]
