"""CPU: the surface of EQTransformer's decoder training step (vp_eqt_dec_train_*, EQTransformerDecoderTrainer,
EQTransformerLit(trainable=...)) and the single-stage numpy formulas of tests/eqt_dec_restate.py against float64 autograd, with
the planted faults the GPU bars must see."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eqt_dec_restate as R
from volpick_amd import _lib
from volpick_amd import train as TR

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("create", "destroy", "set_hyper", "step", "step_bank", "step_bank_aug", "read", "write_weights", "tensor_count",
           "tensor_info", "tensor_read", "synchronize", "launch_count", "param_count", "param_name", "param_size", "weight_count",
           "stream", "set_timing", "phase_ms")


def test_the_new_symbols_are_declared_exported_and_bound(lib):
    hdr = (ROOT / "include" / "volpick_hip.h").read_text()
    for short in SYMBOLS:
        name = "vp_eqt_dec_train_" + short
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
        assert decl, f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        n_args = 0 if decl.group(1).strip() == "void" else decl.group(1).count(",") + 1
        assert len(argtypes) == n_args, name
    # the bank entry points take the arguments of the plan-row one, the rows of another type
    assert _lib.SIGNATURES["vp_eqt_dec_train_step_bank"][1] == _lib.SIGNATURES["vp_eqt_dec_train_step_bank_aug"][1]


def test_the_48_tensors_are_the_decoder_rows_of_the_blob_table_in_its_order(lib):
    kind = _lib.VP_MODEL_EQTRANSFORMER
    table = [(lib.vp_param_name(kind, i).decode(), int(lib.vp_param_size(kind, i))) for i in range(lib.vp_param_count(kind))]
    want = [(k, n) for k, n in table if R.is_decoder_key(k)]
    got = TR.decoder_param_names()
    assert got == want and len(got) == 48
    assert sum(n for _, n in got) == R.N_FLOATS == lib.vp_eqt_dec_train_weight_count() == 145731
    # per decoder: seven (weight, bias) pairs of the stage shapes, then the head after decoder_d / after both pick decoders
    names = [k for k, _ in got]
    assert names[:16] == [f"decoder_d.convs.{i}.{w}" for i in range(7) for w in ("weight", "bias")] + ["conv_d.weight", "conv_d.bias"]
    assert names[-4:] == ["pick_convs.0.weight", "pick_convs.0.bias", "pick_convs.1.weight", "pick_convs.1.bias"]
    sizes = dict(got)
    for d in R.DEC_PREFIX:
        for i in range(7):
            assert sizes[f"{d}.convs.{i}.weight"] == R.DCO[i] * R.DCI[i] * R.DK[i] and sizes[f"{d}.convs.{i}.bias"] == R.DCO[i]
    assert lib.vp_eqt_dec_train_param_name(48) is None and lib.vp_eqt_dec_train_param_size(-1) == 0
    # the restatement's module holds the same 48 tensors
    assert sorted(k for k, _ in R.DecoderHeads().named_parameters()) == sorted(names)


def test_trainable_is_validated_and_the_default_still_raises():
    model = object.__new__(TR.EQTransformer)
    model.in_samples = 6000
    lit = TR.EQTransformerLit(model=model)
    assert lit.trainable is None
    with pytest.raises(NotImplementedError, match="trainable='decoders'"):
        lit.training_step({"X": None, "y": None, "detections": None})
    with pytest.raises(NotImplementedError):
        lit.fit_bank(None, 1)
    for bad in ("all", "trunk", "decoder", True, 1):
        with pytest.raises(ValueError, match="'decoders'"):
            TR.EQTransformerLit(model=model, trainable=bad)
    lit = TR.EQTransformerLit(model=model, trainable="decoders", lr=1e-3)
    assert lit.trainable == "decoders" and lit._trainer is None  # (the trainer is made by the first step: it needs the GPU)
    assert [lit.learning_rate(s) for s in (0, 1, 250, 500, 900)] == [1e-3, 1e-3 / 500, 1e-3 * 250 / 500, 1e-3, 1e-3]
    with pytest.raises(TypeError, match="EQTransformer"):
        TR.EQTransformerDecoderTrainer(object())


def test_fit_scheduler_checks_are_shared_by_both_lits():
    with pytest.raises(ValueError, match="lr_scheduler must be None or one of"):
        TR._fit_scheduler("StepLR", None, object(), False, None)
    for kw in (dict(lr_scheduler="ReduceLROnPlateau"), dict(keep_best=True), dict(early_stop_patience=2)):
        args = dict(lr_scheduler=None, lr_scheduler_args=None, val_bank=None, keep_best=False, early_stop_patience=None)
        args.update(kw)
        with pytest.raises(ValueError, match="need val_bank"):
            TR._fit_scheduler(**args)
    s = TR._fit_scheduler("ReduceLROnPlateau", {"factor": 0.5, "patience": 0}, object(), False, None)
    assert isinstance(s, TR.ReduceLROnPlateau) and s.factor == 0.5
    assert TR._fit_scheduler(None, None, None, False, None) is None


# ---- the single-stage formulas ---------------------------------------------------------------------------------------------
STAGE = 2  # the cropped stage: 64 -> 32 channels, K = 5, 188 -> 375 samples
B = 2


@pytest.fixture(scope="module")
def stage():
    rng = np.random.default_rng(5)
    ci, co, k, lin, lout = R.DCI[STAGE], R.DCO[STAGE], R.DK[STAGE], R.DIN[STAGE], R.DOUT[STAGE]
    x = np.maximum(rng.standard_normal((B, ci, lin)), 0.0)  # what a stage reads is behind a ReLU: exact zeros included
    w = rng.standard_normal((co, ci, k)) / np.sqrt(ci * k)
    b = 0.1 * rng.standard_normal(co)
    ga = rng.standard_normal((B, co, lout))
    xt, wt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, w, b))
    u = F.interpolate(xt, scale_factor=2, mode="nearest")[:, :, :lout]
    a = torch.relu(F.conv1d(u, wt, bt, padding=k // 2))
    (a * torch.tensor(ga)).sum().backward()
    auto = {"a": a.detach().numpy(), "ga_in": xt.grad.numpy(), "gw": wt.grad.numpy(), "gb": bt.grad.numpy()}
    return dict(x=x, w=w, b=b, ga=ga, lout=lout, auto=auto, n_in=co * k + 1, n_w=B * lout)


def test_the_stage_formulas_equal_float64_autograd(stage):
    a, abs_a = R.stage_forward(stage["x"], stage["w"], stage["b"], stage["lout"])
    auto = stage["auto"]
    assert (a == 0).mean() > 0.2 and np.abs(a - auto["a"]).max() < 1e-13
    assert np.all(abs_a >= np.abs(a))
    back = R.stage_backward(stage["x"], a, stage["ga"], stage["w"], stage["lout"])
    for key in ("ga_in", "gw", "gb"):
        scale = np.abs(auto[key]).max()
        assert np.abs(back[key] - auto[key]).max() < 1e-12 * scale, key
        assert np.all(back["abs_" + key] >= np.abs(back[key]) * (1 - 1e-12)), key
    # the crop: the last input sample has ONE up-sampled copy
    assert back["ga_in"].shape[-1] == 188 and np.abs(back["ga_in"][..., 187]).max() > 0


@pytest.mark.parametrize("fault, key", [("crop", "ga_in"), ("mask_ge", "ga_in"), ("drop_tap", "ga_in"), ("drop_tap", "gw"),
                                        ("bias_one_window", "gb")])
def test_a_planted_fault_exceeds_the_fp32_bar(stage, fault, key):
    a, _ = R.stage_forward(stage["x"], stage["w"], stage["b"], stage["lout"])
    right = R.stage_backward(stage["x"], a, stage["ga"], stage["w"], stage["lout"])
    wrong = R.stage_backward(stage["x"], a, stage["ga"], stage["w"], stage["lout"], fault=fault)
    n = stage["n_in"] if key == "ga_in" else stage["n_w"]
    bar = R.gamma(n) * right["abs_" + key]
    err = np.abs(wrong[key] - right[key])
    assert err.max() > 0 and (err / bar).max() > 100, (fault, key, (err / bar).max())
    if fault == "crop":  # ... and shows exactly where it is planted: j = 187 of every row, nowhere else
        assert np.all(err[..., :187] == 0) and (err[..., 187] / bar[..., 187]).min() > 1
    if fault == "drop_tap" and key == "gw":
        assert np.all(err[:, :, :-1] == 0)


def test_the_head_formulas_equal_float64_autograd():
    rng = np.random.default_rng(6)
    a6 = np.maximum(rng.standard_normal((B, 8, 300)), 0.0)
    w, b = rng.standard_normal((1, 8, 11)) / 9.0, rng.standard_normal(1)
    y = rng.random((B, 300))
    at, wt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (a6, w, b))
    z = F.conv1d(at, wt, bt, padding=5)[:, 0]
    p = torch.sigmoid(z)
    p.retain_grad(), z.retain_grad()
    loss = 0.4 * torch.nn.BCELoss()(p, torch.tensor(y))
    loss.backward()
    z64, abs_z = R.head_forward(a6, w, b)
    assert np.abs(z64 - z.detach().numpy()).max() < 1e-13 and np.all(abs_z >= np.abs(z64) - 1e-15)
    assert np.abs(R.sigmoid(z64) - p.detach().numpy()).max() < 1e-15
    gz = R.head_gradient(p.detach().numpy(), y, 0.4, B * 300)
    # (the restatement rounds the weight and the count to fp32 as the kernel holds them: 0.4 is not a float32)
    assert np.abs(gz - z.grad.numpy()).max() < 1e-7 * np.abs(gz).max()
    back = R.head_backward(z.grad.numpy(), a6, w)
    for key, want in (("ga6", at.grad.numpy()), ("gw", wt.grad.numpy()), ("gb", bt.grad.numpy())):
        assert np.abs(back[key] - want).max() < 1e-12 * np.abs(want).max(), key


def test_edge_samples_name_the_crop():
    assert R.edge_samples(375, 5) == [0, 1, 373, 374]
    assert R.edge_samples(94, 3) == [0, 93] and R.edge_samples(6000, 11) == [0, 1, 2, 3, 4, 5995, 5996, 5997, 5998, 5999]
    assert R.gamma(321) == pytest.approx(321 * 2.0 ** -24, rel=1e-4)
