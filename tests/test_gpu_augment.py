"""GPU: augmented training windows (stacked events and noise, Gaussian noise, gap, second normalisation) generated from
a device-resident waveform bank (csrc/batchgen.hip, bank_aug_kernel<3, LABEL_PSN>) against the float64 restatement of their records
(tests/augment_restate.py), invalid records, and the fused trainer path (vp_train_step_bank_aug) against ``step``."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from volpick_amd import PhaseNet, _lib
from volpick_amd import generate as G
from volpick_amd.train import PhaseNetLit, PhaseNetTrainer
from tests import augment_restate as R
from tests.test_gpu_generate import build_traces, synthetic_bank

pytestmark = pytest.mark.gpu

T = 3001
CASES = {
    "reference": {},
    "superimpose": dict(event_prob=(1, 0, 0), noise_prob=(0, 0, 1), gap_prob=(0, 1)),
    "two_events": dict(event_prob=(1, 0, 0), noise_prob=(0, 0, 1), gap_prob=(0, 1), prob_num_events={2: 1.0}),
    "duplicate": dict(event_prob=(0, 1, 0), noise_prob=(0, 0, 1), gap_prob=(0, 1), prob_num_events={2: 1.0}),
    "noise": dict(event_prob=(0, 0, 1), noise_prob=(1, 0, 0), gap_prob=(0, 1), prob_num_events={2: 1.0}),
    "gauss": dict(event_prob=(0, 0, 1), noise_prob=(0, 1, 0), gap_prob=(0, 1)),
    "gap": dict(event_prob=(0, 0, 1), noise_prob=(0, 0, 1), gap_prob=(1, 0)),
    "events_noise_gap": dict(event_prob=(1, 1, 0), noise_prob=(1, 1, 0), gap_prob=(1, 0)),
}


@pytest.fixture(scope="module")
def setup():
    traces, onsets = build_traces()
    # extra event traces whose P lies well inside a 1500-sample lead, so that sources pass the P-label check
    rng = np.random.default_rng(0)
    for i in range(6):
        L = 7000 + 500 * i
        x = rng.standard_normal((3, L)).astype(np.float32) * (0.5 + i)
        p = 2000.0 + 137.3 * i
        x[:, int(p):int(p) + 600] *= 8
        if i == 2:
            x[2] = 0.0  # an all-zero channel
        traces.append(x)
        onsets = np.vstack([onsets, [p, np.nan, p + 700.25, np.nan]])
    bank = G.WaveformBank(traces, {"P": onsets[:, :2], "S": onsets[:, 2:]})
    yield traces, onsets, bank
    bank.close()


def check(got_x, got_y, rows, traces, onsets, sigma, norm, labels):
    gx, gy = got_x.cpu().numpy().astype(np.float64), got_y.cpu().numpy().astype(np.float64)
    for b, rec in enumerate(rows):
        wx, wy = R.execute(rec, traces, onsets, T, sigma, norm, labels)
        scale = 1.0 if norm == "peak" else max(np.abs(wx).max(), 1e-30)
        ex = np.abs(gx[b] - wx).max() / scale
        assert ex <= 4e-6, (b, ex, rec)
        ey = np.abs(gy[b] - wy).max()
        assert ey <= 1e-6, (b, ey, rec)


def planned(bank, B, seed, kw, sigma=20):
    n = bank.n_traces
    planner = G.AugmentedPlanner(bank, B, np.arange(8, n), np.arange(0, 8), seed=seed, sigma=sigma, **kw)
    return planner.plan(np.random.default_rng(seed).integers(0, n, B))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("norm", ["peak", "std"])
def test_kernel_matches_the_restatement(setup, case, norm):
    traces, onsets, bank = setup
    rows = planned(bank, 64, 1, CASES[case])
    model = SimpleNamespace(in_samples=T, labels="PSN", norm=norm)
    out = bank.make_batch(rows, model, 20)
    torch.cuda.synchronize()
    check(out["X"], out["y"], rows, traces, onsets, 20, norm, "PSN")


@pytest.mark.parametrize("B", [1, 7, 512])
@pytest.mark.parametrize("labels", ["PSN", "NPS"])
def test_kernel_batch_sizes_and_label_orders(setup, B, labels):
    traces, onsets, bank = setup
    rows = planned(bank, B, B, CASES["events_noise_gap"] if B < 512 else {})
    model = SimpleNamespace(in_samples=T, labels=labels, norm="std")
    out = bank.make_batch(rows, model, 20)
    torch.cuda.synchronize()
    check(out["X"], out["y"], rows, traces, onsets, 20, "std", labels)


def hand_records(traces):
    """A zero channel in the primary, sources straddling either trace end, a shift of zero, Gaussian noise alone."""
    def row(tr, start):
        return (tr, 0, start, 0, traces[tr].shape[1])

    recs = np.zeros(5, G.AUG_ROW)
    recs["cut"] = T
    recs[0]["primary"] = row(6, 100)  # trace 6 has a constant channel: zero after demeaning
    recs[0]["event"][0] = (row(9, -1200), G.AUG_BANK, 0, 0, 0.5)  # straddles the start of trace 9, shift 0
    recs[1]["primary"] = row(8, 1000)
    recs[1]["cut"] = 2100
    recs[1]["event"][0] = (row(10, traces[10].shape[1] - 1800), G.AUG_BANK, 400, 1500, 1.5)  # straddles the end
    recs[1]["event"][1] = (row(11, 500), G.AUG_BANK, 700, -900, 0.3)
    recs[2]["primary"] = row(12, 900)
    recs[2]["event"][0] = ((0, 0, 0, 0, 0), G.AUG_SELF, 900, 0, 2.0)
    recs[2]["noise"][0] = (row(1, 3000), G.AUG_BANK, 0.1)
    recs[2]["noise"][1] = (row(13, -500), G.AUG_BANK, 0.02)
    recs[3]["primary"] = row(3, 4000)
    recs[3]["gauss"] = 0.1
    recs[3]["noise_key"] = 0x0123456789ABCDEF
    recs[4]["primary"] = row(0, 2000)
    recs[4]["event"][0] = (row(10, 0), G.AUG_BANK, 0, -T, 1.0)  # wholly outside: labels renormalise only
    recs[4]["gap_lo"], recs[4]["gap_hi"] = 10, 2990
    return recs


@pytest.mark.parametrize("norm", ["peak", "std"])
def test_hand_made_records(setup, norm):
    traces, onsets, bank = setup
    recs = hand_records(traces)
    model = SimpleNamespace(in_samples=T, labels="PSN", norm=norm)
    out = bank.make_batch(recs, model, 20)
    torch.cuda.synchronize()
    check(out["X"], out["y"], recs, traces, onsets, 20, norm, "PSN")


def test_gaussian_noise_draws(setup):
    """The kernel's draws equal the numpy Philox4x32-10 / Box-Muller restatement: the same window without and with
    Gaussian noise, the difference restated from the first."""
    traces, onsets, bank = setup
    recs = np.zeros(2, G.AUG_ROW)
    recs["cut"] = T
    recs["primary"] = [(3, 0, 4000, 0, traces[3].shape[1])] * 2
    recs[1]["gauss"] = 0.125
    recs[1]["noise_key"] = 0xFEDCBA9876543210
    model = SimpleNamespace(in_samples=T, labels="PSN", norm="peak")
    plain = bank.make_batch(recs[:1], model, 20)["X"][0].cpu().numpy().astype(np.float64)
    out = bank.make_batch(recs[1:], model, 20)["X"][0].cpu().numpy().astype(np.float64)
    noisy = plain + 0.125 * plain.max() * R.gauss_noise(recs[1]["noise_key"], T)
    want = R.normalise(noisy, "peak")
    assert np.abs(out - want).max() <= 4e-6


def raw(bank, rows, x, y, T_=T):
    lr = (C.c_int * 3)(0, 1, 2)
    rows = np.ascontiguousarray(rows)
    return _lib.load().vp_bank_make_batch_aug(bank.handle, rows.ctypes.data_as(C.c_void_p), len(rows), T_, 20.0,
                                              _lib.VP_NORM_PEAK, lr, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_invalid_records_raise_and_leave_the_outputs_untouched(setup):
    traces, onsets, bank = setup
    good = hand_records(traces)
    bad = []

    def variant(f):
        r = good.copy()
        f(r)
        bad.append(r)

    variant(lambda r: r[0]["event"].__setitem__(0, ((99, 0, 0, 0, 10), G.AUG_BANK, 0, 0, 1.0)))  # trace out of range
    variant(lambda r: r[1]["event"].__setitem__(0, ((10, 0, 0, 0, 10 ** 7), G.AUG_BANK, 0, 0, 1.0)))  # hi past the trace
    variant(lambda r: r[1]["event"].__setitem__(1, ((11, 0, 0, 0, 10), G.AUG_BANK, 0, T + 1, 1.0)))  # |shift| > T
    variant(lambda r: r[2]["event"].__setitem__(0, ((0, 0, 0, 0, 0), G.AUG_SELF, 0, 0, -1.0)))  # negative scale
    variant(lambda r: r[2]["noise"].__setitem__(0, ((1, 0, 0, 0, 10), G.AUG_BANK, np.inf)))  # non-finite scale
    variant(lambda r: r[3].__setitem__("gap_lo", 20) or r[3].__setitem__("gap_hi", 10))  # gap_lo > gap_hi
    variant(lambda r: r[3].__setitem__("cut", T + 1))
    variant(lambda r: r[0]["event"].__setitem__(1, ((0, 0, 0, 0, 0), G.AUG_NONE, 0, 5, 0.0)))  # unused, not zero
    variant(lambda r: r[0]["noise"].__setitem__(1, ((0, 0, 0, 0, 0), 3, 0.0)))  # kind out of range
    variant(lambda r: r[4].__setitem__("noise_key", 7))  # a key without Gaussian noise
    variant(lambda r: r[2]["event"].__setitem__(0, ((1, 0, 0, 0, 0), G.AUG_SELF, 0, 0, 1.0)))  # self with a row
    x = torch.full((5, 3, T), 7.0, device="cuda")
    y = torch.full((5, 3, T), 7.0, device="cuda")
    model = SimpleNamespace(in_samples=T, labels="PSN", norm="peak")
    for r in bad:
        assert raw(bank, r, x, y) == -1  # VP_ERR_INVALID
        with pytest.raises(_lib.VolpickHipError):
            bank.make_batch(r, model, 20)
    assert raw(bank, good, x, y, T_=3073) == -1
    torch.cuda.synchronize()
    assert (x == 7).all() and (y == 7).all()
    assert raw(bank, good, x, y) == 0
    torch.cuda.synchronize()
    assert not (x == 7).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_bank_aug_matches_step_bit_for_bit(dtype):
    B = 64
    w, ps, ss, bank = synthetic_bank(96, seed=3, device_tensor=True)
    try:
        a = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B, dtype=dtype)
        b = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B, dtype=dtype)
        model = a.model
        planner = G.AugmentedPlanner(bank, B, np.arange(0, 64), np.arange(64, 96), seed=5, sigma=20,
                                     event_prob=(1, 1, 1), noise_prob=(1, 1, 1), gap_prob=(1, 1))
        plans = [rows for _ in range(3) for rows in planner.epoch()]
        assert len(plans) == 3 and (plans[0]["event"]["kind"] != 0).any()
        for k, rows in enumerate(plans):
            batch = bank.make_batch(rows, model, 20)
            la = a.step_bank(bank, rows, lr=1e-3, sigma=20)
            lb = b.step(batch["X"], batch["y"], lr=1e-3)
            assert la == lb, (k, la, lb)
        wa, wb = a.weights(), b.weights()
        for key in wa:
            assert np.array_equal(wa[key], wb[key]), key
        xa, xb = a.tensors(B)["x"], b.tensors(B)["x"]
        assert np.array_equal(xa, xb)
        if dtype == "fp32":
            assert np.array_equal(xa, batch["X"].cpu().numpy())
        a.close()
        b.close()
    finally:
        bank.close()


def test_fit_bank_with_augmentation_learns():
    from oracle.models import PhaseNet as TorchPhaseNet

    torch.manual_seed(2)
    net = TorchPhaseNet(phases="PSN", norm="peak")
    model = PhaseNet(phases="PSN", norm="peak")
    model.load_state_dict({k: v.detach().numpy() for k, v in net.state_dict().items()})
    _, _, _, bank = synthetic_bank(256, L=9000, seed=11)
    _, _, _, val = synthetic_bank(40, L=9000, seed=12)
    try:
        aug = G.Augmentation(event_traces=np.arange(0, 200), noise_traces=np.arange(200, 256),
                             val_event_traces=np.arange(0, 30), val_noise_traces=np.arange(30, 40))
        lit = PhaseNetLit(lr=1e-2, model=model, max_batch=64, precision="bf16-mixed")
        losses, val_losses = lit.fit_bank(bank, 50, batch_size=64, seed=0, val_bank=val, augment=aug)
        losses = np.array(losses)
        assert len(losses) == 50 and np.isfinite(losses).all()
        assert losses[-10:].mean() < losses[:10].mean(), losses
        assert len(val_losses) == 13 and np.isfinite(val_losses).all()
    finally:
        bank.close()
        val.close()
