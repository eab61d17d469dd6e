"""CPU: EQTransformer's batch and loss without a device.  The restated detection rule on adversarial onsets against slices
worked out by hand; the five new entry points declared, exported and bound with the header's argument counts, and their
null arguments refused; ``train.bce_loss`` and the longdouble truth against ``torch.nn.BCELoss``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import volpick_amd
from tests import eqt_batch_restate as R
from volpick_amd import _lib
from volpick_amd import generate as G
from volpick_amd import train as TR

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "volpick_hip.h").read_text()
NAMES = ["vp_bank_make_batch_eqt", "vp_bce_loss", "vp_validate_eqt_begin", "vp_validate_eqt_bank", "vp_validate_eqt_end"]


# ---------------------------------------------------------------------------------------------------- the detection rule
def test_the_rule_is_named_in_generate():
    assert G.DETECTION_FACTOR == 1.4 and G.DETECTION_ONSET == "earliest" and G.DETECTION_INDEX is np.trunc
    assert G.DETECTION_NEEDS == "P and S" and G.DETECTION_ORDER == "s >= p"


@pytest.mark.parametrize("T", [6000, 1025, 7])
@pytest.mark.parametrize("case", R.ADVERSARIAL_ONSETS, ids=[c[0] for c in R.ADVERSARIAL_ONSETS])
def test_detection_rule_on_adversarial_onsets(case, T):
    _, onsets, fixed, (p0, p1) = case
    want = np.zeros(T)
    want[p0:p1] = 1  # the slice clips p1 (and p0) beyond T
    got = R.detection_row(np.array(onsets), T, fixed)
    assert np.array_equal(got, want), (np.flatnonzero(got)[[0, -1]] if got.any() else None, (p0, p1))
    assert set(np.unique(got)) <= {0.0, 1.0}


def test_the_end_index_rounds_its_product_before_its_sum():
    """p = -2304, s = -1101.5: Python's s + 1.4 * (s - p) is exactly 582.0; one rounding (a fused multiply-add) gives
    581.9999999999999 and the slice would end a sample early."""
    p, s = -2304.0, -1101.5
    assert s + 1.4 * (s - p) == 582.0
    exact = np.longdouble(s) + np.longdouble(1.4) * np.longdouble(s - p)  # the product unrounded: what an fma adds
    assert float(exact) == 581.9999999999999 and int(float(exact)) == 581
    row = R.detection_row(np.array([p, np.nan, s, np.nan]), 6000)
    assert row[:582].all() and not row[582:].any()


def test_label_row_helpers():
    assert list(G.detection_label_rows(["Detection", "P", "S"])) == [0, 1, 2]
    assert list(G.detection_label_rows(["P", "S", "Detection"])) == [2, 0, 1]
    assert G.has_detection_row(["Detection", "P", "S"]) and not G.has_detection_row("PSN") and not G.has_detection_row("NPS")
    with pytest.raises(ValueError):
        G.detection_label_rows("PSN")
    with pytest.raises(ValueError):
        G._fixed_window(-1)
    assert G._fixed_window(None) == -1.0 and G._fixed_window(250.5) == 250.5


# ------------------------------------------------------------------------------------------------------------ the symbols
def test_symbols_are_declared_exported_and_bound(lib):
    for name in NAMES:
        m = re.search(r"^int " + name + r"\(([^;]*)\);", HEADER, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("EQTransformerLit", "bce_loss", "validate_batches_eqt"):
        assert getattr(volpick_amd, name) is getattr(TR, name)


def test_null_arguments_are_refused_without_a_device(lib):
    rows = np.zeros(2, G.PLAN_ROW)
    lrows = (C.c_int * 3)(0, 1, 2)
    w = (C.c_double * 3)(*R.WEIGHTS)
    out = np.full(8, -77.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.vp_bank_make_batch_eqt(None, p(rows), 2, 6000, 20.0, 0, lrows, -1.0, None, None, None) == -1
    assert b"null" in lib.vp_last_error()
    assert lib.vp_bce_loss(0, None, None, 2, 3, 64, w, p(out), p(out), p(out), None) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_validate_eqt_begin(None) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_validate_eqt_bank(None, None, p(rows), 2, 20.0, 0, lrows, -1.0, w, None) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_validate_eqt_end(None, dp(out), 1, None, dp(out), dp(out), 1, None) == -1 and b"null" in lib.vp_last_error()
    assert (out == -77.0).all()


# ---------------------------------------------------------------------------------------------------------------- the loss
def torch_loss(p, y, weights, dtype):
    """The reference's shared_step sum (models.py:545-549) generalised to C rows: sum_c w_c BCELoss(p[:, c], y[:, c])."""
    loss = torch.nn.BCELoss()
    pt, yt = torch.from_numpy(p).to(dtype), torch.from_numpy(y).to(dtype)
    return float(sum(float(w) * loss(pt[:, c], yt[:, c]).double() for c, w in enumerate(weights)))


@pytest.mark.parametrize("kind", R.INPUT_KINDS)
@pytest.mark.parametrize("shape", [(3, 3, 6000), (5, 3, 3001), (3, 1, 7)])
def test_bce_loss_equals_torch(kind, shape):
    p, y = R.make_inputs(kind, shape, seed=3)
    w = R.weights_for(shape[1])
    got = TR.bce_loss(p, y, w)
    heads, windows, batch, _ = R.bce_truth(p, y, w)
    head_bar, window_bar, batch_bar = R.bars(p, y, w)
    want64 = torch_loss(p, y, w, torch.float64)
    print(f"{kind} {shape}: bce_loss {got!r}, torch float64 {want64!r}, truth {batch!r}, bar {batch_bar:.3g}")
    assert np.isfinite(got) and got > 0
    assert abs(got - want64) <= 2 * batch_bar  # each side's own float64 rounding
    assert abs(got - batch) <= batch_bar and abs(want64 - batch) <= batch_bar
    got_heads = TR.bce_heads(p, y)
    assert (np.abs(got_heads - heads) <= head_bar).all()
    assert (np.abs((got_heads * w).sum(-1) - windows) <= window_bar).all()
    # ... and the fp32 loss the reference calls is this number at fp32's precision
    want32 = torch_loss(p, y, w, torch.float32)
    assert abs(got - want32) <= 1e-6 * abs(want32), (got, want32)
    if kind == "clamped":  # the stretches of exactly 100 are in the sum
        assert heads.min() > 100.0 * (max(1, shape[2] // 4) * 2) / shape[2] * 0.99


def test_bce_loss_propagates_non_finite_values_as_torch_does():
    p, y = R.make_inputs("sigmoid", (4, 3, 64), seed=1)
    p[1, 2, 5] = np.nan
    p[2, 0, 7] = 1.5  # outside [0, 1]: log(1 - p) is NaN
    heads = TR.bce_heads(p, y)
    assert np.isnan(heads[1, 2]) and np.isnan(heads[2, 0]) and np.isfinite(np.delete(heads.ravel(), [5, 6])).all()
    assert np.isnan(TR.bce_loss(p, y, R.WEIGHTS))
    with pytest.raises(ValueError):
        TR.bce_loss(p, y, (1.0, 1.0))


def test_eqtransformer_lit_without_a_device():
    lit = TR.EQTransformerLit(model=object.__new__(TR.EQTransformer))
    lit.model.in_samples = 6000
    assert lit.loss_weights == (0.05, 0.40, 0.55) and lit.sigma == 20 and lit.detection_fixed_window is None
    with pytest.raises(NotImplementedError):
        lit.training_step({})
    with pytest.raises(ValueError, match="gaussian"):
        TR.EQTransformerLit(prob_label_shape="triangle", model=lit.model)
    bank = type("B", (), {"lengths": np.full(5, 20000), "onsets": np.tile([9000.0, np.nan, 9800.0, np.nan], (5, 1))})()
    pl = lit.window_planner(bank, 4, seed=1)
    assert (pl.samples_before, pl.first_windowlen, pl.in_samples, pl.batch_size) == (6000, 12000, 6000, 4)
    rows = pl.plan(np.arange(5))
    assert ((rows["hi"] - rows["lo"] == 12000) | (rows["hi"] - rows["lo"] == 20000)).all()
