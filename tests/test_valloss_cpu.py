"""CPU: the float64 oracle of the validation-loss tests against the reference's formula in torch, the torch-free
ReduceLROnPlateau against torch's on seeded loss sequences, its interaction with the warm-up against a restatement on a
real Adam parameter group, and the argument checks of ``PhaseNetLit.fit_bank``."""
import itertools

import numpy as np
import pytest
import torch

from tests import valloss_f64 as V
from volpick_amd import train as TR


def reference_formula(y_pred, y_true, eps=1e-5):
    """volpick/model/models.py:43-51 of the reference, on float64 tensors."""
    h = y_true * torch.log(y_pred + eps)
    h = h.mean(-1).sum(-1)
    return -h.mean(), -h


@pytest.mark.parametrize("kind", V.INPUT_KINDS)
@pytest.mark.parametrize("shape", [(5, 3, 3001), (3, 1, 7)])
def test_oracle_equals_the_reference_formula_in_torch_float64(kind, shape):
    p, y = V.make_inputs(kind, shape, seed=3)
    want_batch, want = reference_formula(torch.from_numpy(p).double(), torch.from_numpy(y).double())
    got = V.per_window_loss(p, y)
    scale = np.abs(want.numpy()).max()
    assert np.abs(got - want.numpy()).max() <= 1e-15 * scale
    assert abs(got.mean() - float(want_batch)) <= 1e-15 * scale
    # ... and the package's own host loss is that number
    assert abs(TR.vector_cross_entropy(p.astype(np.float64), y.astype(np.float64)) - float(want_batch)) <= 1e-15 * scale
    assert (V.bar(p, y) >= 0).all() and V.batch_bar(p, y) >= 0
    if kind == "y_zero":
        assert (got == 0).all() and (V.bar(p, y) == 0).all()


@pytest.mark.parametrize("misalign", [None, 0, 3])
def test_the_kernels_summation_order_stays_far_inside_the_bar(misalign):
    """Where the bar comes from: the kernel's order (per-thread strided partials, halving folds) against numpy's pairwise
    sums and against math.fsum, on softmax-like inputs, is a small fraction of it."""
    import math

    p, y = V.make_inputs("softmax", (5, 3, 3001), seed=1)
    got = V.kernel_order_loss(p, y, misalign=misalign)
    want = V.per_window_loss(p, y)
    exact = np.array([-math.fsum((y[b].astype(np.float64) * np.log(p[b].astype(np.float64) + 1e-5)).ravel()) / 3001
                      for b in range(5)])
    bar = V.bar(p, y)
    assert (np.abs(got - want) <= 1e-3 * bar).all(), np.abs(got - want) / bar
    assert (np.abs(got - exact) <= 1e-3 * bar).all(), np.abs(got - exact) / bar
    assert (np.abs(want - exact) <= 1e-3 * bar).all()


GRID = list(itertools.product((0.5, 0.1), (0, 1, 20), (0, 2), (0.0, 1e-6)))


def test_reduce_lr_on_plateau_equals_torch_on_200_sequences():
    seqs = V.loss_sequences(200, 60, seed=7)
    n_reductions = 0
    for i, seq in enumerate(seqs):
        factor, patience, cooldown, min_lr = GRID[i % len(GRID)]
        lr0 = (1e-2, 5e-4, 3e-6)[i % 3]
        args = dict(factor=factor, patience=patience, cooldown=cooldown, min_lr=min_lr)
        want = V.torch_plateau_lrs(seq, lr0, **args)
        sched = TR.ReduceLROnPlateau(**args)
        lr, got = lr0, []
        for v in seq:
            lr = sched.step(v, lr)
            got.append(lr)
        assert got == want, (i, args)
        n_reductions += len(set(got))
    assert n_reductions > 400  # the sequences do reduce
    # every cell of the grid was used with every kind of sequence
    assert len(seqs) >= 4 * len(GRID)


def test_reduce_lr_on_plateau_skips_a_reduction_below_eps_and_knows_abs_mode():
    want = V.torch_plateau_lrs([1.0] * 6, 1.5e-8, factor=0.5, patience=0, min_lr=0.0)
    sched, lr, got = TR.ReduceLROnPlateau(factor=0.5, patience=0, min_lr=0.0), 1.5e-8, []
    for _ in range(6):
        lr = sched.step(1.0, lr)
        got.append(lr)
    assert got == want and got[-1] == 1.5e-8  # 1.5e-8 - 0.75e-8 <= eps = 1e-8: never reduced
    seq = [1.0, 0.99, 0.985, 0.98, 0.98, 0.97, 0.97, 0.97]
    args = dict(factor=0.1, patience=1, threshold=0.01, threshold_mode="abs", cooldown=1, min_lr=1e-5)
    sched, lr, got = TR.ReduceLROnPlateau(**args), 1e-2, []
    for v in seq:
        lr = sched.step(v, lr)
        got.append(lr)
    assert got == V.torch_plateau_lrs(seq, 1e-2, **args)
    with pytest.raises(ValueError):
        TR.ReduceLROnPlateau(factor=1.0)


class StubTrainer:
    """Counts steps and records their learning rates: what fit_bank needs of a PhaseNetTrainer, without a GPU."""

    def __init__(self):
        self.global_step, self.forward_count, self.lrs = 0, 0, []

    def step_bank(self, bank, rows, lr, sigma, update=True, want_loss=True):
        self.lrs.append(lr)
        self.global_step += 1
        self.forward_count += 1
        return 1.0 / self.global_step

    def weights(self):
        return {"w": np.array([float(self.global_step)])}


class StubBank:
    def __init__(self, n):
        self.lengths = np.full(n, 9000, np.int64)
        self.onsets = np.full((n, 4), np.nan)
        self.onsets[:, 0] = 4000.0


def stub_lit(monkeypatch, val_losses, **kw):
    lit = TR.PhaseNetLit(model=object.__new__(TR.PhaseNet), **kw)
    lit.model.in_samples = 3001
    lit._trainer = StubTrainer()
    feed = iter(val_losses)
    monkeypatch.setattr(lit, "validate_bank", lambda bank, planner: [next(feed)])
    return lit


@pytest.mark.parametrize("sched_args", [dict(factor=0.5, patience=0, min_lr=1e-6), dict(factor=0.1, patience=1, min_lr=0.0)])
def test_warmup_and_scheduler_share_one_learning_rate(monkeypatch, sched_args):
    """WARMUP_STEPS = 8, epochs of 3 steps: reductions made inside the warm-up are overwritten by its next step, reductions
    after it persist and compound."""
    val = [1.0, 1.1, 1.2, 0.9, 0.95, 0.96, 0.97, 0.5, 0.6, 0.7]
    lit = stub_lit(monkeypatch, val, lr=1e-2)
    lit.WARMUP_STEPS = 8
    losses, val_losses = lit.fit_bank(StubBank(3 * 4 + 2), 28, batch_size=4, val_bank=StubBank(5), validation="device",
                                      lr_scheduler="ReduceLROnPlateau", lr_scheduler_args=sched_args)
    used, after = V.torch_warmup_plateau(1e-2, 8, 28, 3, val, **sched_args)
    assert len(losses) == 28 and val_losses == val  # 9 epoch ends and the last step
    assert lit._trainer.lrs == used
    assert lit.history["lr"] == after
    # a reduction in the warm-up was overwritten, and later ones persisted
    if sched_args["patience"] == 0:  # validation 1 (after step 5) halves 1e-2 * 6 / 8 for step 6 alone
        assert after[1] == used[6] == 0.5 * (1e-2 * 6 / 8) and used[7] == 1e-2 * 7 / 8
    assert used[8] == 1e-2 and used[-1] == after[-2] < 1e-2
    assert lit.history["best"] == (7, 24, 0.5) and not lit.history["stopped_early"]


def test_without_a_scheduler_the_learning_rates_are_todays(monkeypatch):
    lit = stub_lit(monkeypatch, [1.0] * 20, lr=1e-2)
    lit.WARMUP_STEPS = 8
    lit.fit_bank(StubBank(14), 20, batch_size=4, val_bank=StubBank(5), validation="device")
    assert lit._trainer.lrs == [lit.learning_rate(k) for k in range(20)]
    assert lit.history["lr"] == [lit.learning_rate(k) for k in (3, 6, 9, 12, 15, 18, 20)]


def test_keep_best_and_early_stop(monkeypatch):
    val = [1.0, 0.8, 0.8, 0.9, 0.7]
    lit = stub_lit(monkeypatch, val, lr=1e-2)
    losses, val_losses = lit.fit_bank(StubBank(14), 30, batch_size=4, val_bank=StubBank(5), validation="device",
                                      keep_best=True, early_stop_patience=2)
    # the minimum is the FIRST 0.8 (strictly lower only); two validations without a new one end the fit
    assert val_losses == val[:4] and len(losses) == 12
    assert lit.history["best"] == (1, 6, 0.8) and lit.history["stopped_early"]
    assert lit.best_state["w"][0] == 6.0


def test_fit_bank_argument_errors(monkeypatch):
    lit = stub_lit(monkeypatch, [1.0], lr=1e-2)
    bank = StubBank(14)
    with pytest.raises(ValueError, match="val_bank"):
        lit.fit_bank(bank, 4, batch_size=4, lr_scheduler="ReduceLROnPlateau")
    with pytest.raises(ValueError, match="lr_scheduler"):
        lit.fit_bank(bank, 4, batch_size=4, val_bank=StubBank(5), lr_scheduler="CosineAnnealingLR")
    with pytest.raises(ValueError, match="validation"):
        lit.fit_bank(bank, 4, batch_size=4, val_bank=StubBank(5), validation="gpu")
    with pytest.raises(ValueError, match="val_bank"):
        lit.fit_bank(bank, 4, batch_size=4, keep_best=True)
    assert lit._trainer.global_step == 0
