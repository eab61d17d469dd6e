"""Teeth of the per-layer float64 check (tests/layer_f64.py), on CPU: every conv layer of both models, computed in torch fp32
with the lo piece of its three-piece bf16 operands dropped (weights or input truncated to hi + mid: one lost i + j = 2
product term), must fail the bars the GPU test holds the shipped kernels to -- by a margin, so that the bars cannot be
loosened until they no longer see that fault -- while plain fp32 passes them.

What is measured first is the bare conv (no BatchNorm, no ReLU, unfolded weights; the volpick weights, two windows), a close
neighbour of what the GPU test compares (post-BatchNorm / ReLU outputs of layers whose kernels fold BatchNorm into the weights):
the margin shows the metric's sensitivity to the fault, not the GPU test's exact numbers.  EQTransformer's layers are then
measured through the very descriptors the GPU test uses (tests/layer_f64.eqt_layers).  This runs no kernel: it covers the bars."""
import copy

import pytest
import torch

from oracle import pipeline as OP
from oracle.models import load_pretrained
from tests.layer_f64 import (C_ELEM, EPS24, K_RMS, MID_FAULTS, attention_rows, bf16_drop_lo, elem_scale, eqt_acts, eqt_layers,
                              eqt_mid_acts, eqt_mid_chain, eqt_mid_stages, layer_forward, mid_bad, rel_rms)
from volpick_amd.synthetic import synthetic_windows

MARGIN = 1.75  # the weakest case, EQTransformer pick_convs.0 with its weights' lo piece dropped, sits at 1.8 x K_RMS


def _conv_inputs(net, x):
    ins = {}
    hs = [m.register_forward_hook(lambda mod, i, o, n=n: ins.__setitem__(n, i[0].detach().clone()))
          for n, m in net.named_modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d))]
    with torch.no_grad():
        net(x)
    for h in hs:
        h.remove()
    return ins


@pytest.mark.parametrize("model", ["phasenet", "eqtransformer"])
def test_dropped_lo_piece_fails_the_layer_bars(model):
    net = load_pretrained(model, "volpick")
    x = OP.batch_pre(net, torch.from_numpy(synthetic_windows(2, net.in_samples, seed=3)))
    mods = dict(net.named_modules())
    ins = _conv_inputs(net, x)
    assert len(ins) == {"phasenet": 19, "eqtransformer": 48}[model]
    weak = []
    for name, xin in ins.items():
        conv = mods[name]
        kind = "conv" if isinstance(conv, torch.nn.Conv1d) else "convT"
        with torch.no_grad():
            ref = layer_forward(conv, None, False, kind, xin, torch.float64)
            scale = EPS24 * elem_scale(conv, None, kind, xin)
            r32 = rel_rms(layer_forward(conv, None, False, kind, xin, torch.float32), ref)
            elem = lambda y: float(((y.double() - ref).abs() / (scale + 1e-300)).max())
            e32 = elem(layer_forward(conv, None, False, kind, xin, torch.float32))
            assert e32 <= C_ELEM, (name, e32)  # plain fp32 passes the elementwise bar
            for what, y in (("weights", layer_forward(conv, None, False, kind, xin, torch.float32, weight_fn=bf16_drop_lo)),
                            ("input", layer_forward(conv, None, False, kind, bf16_drop_lo(xin), torch.float32))):
                rr, ee = rel_rms(y, ref) / r32, elem(y)
                # the RMS bar sees the lost term; where the weights are (nearly) exact in two pieces, the elementwise one does
                if not (rr > MARGIN * K_RMS or ee > MARGIN * C_ELEM):
                    weak.append((name, what, round(rr, 2), round(ee, 2)))
    assert not weak, f"{model}: a dropped lo piece passes the per-layer bars (rms ratio, elementwise ratio): {weak}"


def test_dropped_lo_piece_fails_the_eqt_layer_bars():
    """The same over the descriptors the GPU test holds EQTransformer's conv kernels to (tests/layer_f64.eqt_layers: BatchNorm,
    ReLU, max-pool, the residual stream's glue), on the fp32 oracle's own activations.  Exempt: the ResCNN block outputs
    x + conv2(mid) -- the residual stream dilutes the conv's error, and the conv is held to the bars by its increment
    descriptor res.{i}.conv2, which exists for that reason -- and res.act, a BatchNorm without a conv."""
    net = load_pretrained("eqtransformer", "volpick")
    x = OP.batch_pre(net, torch.from_numpy(synthetic_windows(2, net.in_samples, seed=3)))
    acts = eqt_acts(net, x)
    layers = [l for l in eqt_layers(net) if l[4] != "bn" and not (isinstance(l[4], tuple) and l[4][0] == "res")]
    assert len(layers) == 7 + 14 + 3 * 8
    weak, lines = [], []
    for name, conv, bn, relu, kind, inp in layers:
        xin = inp(acts).float()
        with torch.no_grad():
            ref = layer_forward(conv, bn, relu, kind, xin, torch.float64, acts)
            scale = EPS24 * elem_scale(conv, bn, kind, xin, acts)
            elem = lambda y: float(((y.double() - ref).abs() / (scale + 1e-300)).max())
            y32 = layer_forward(conv, bn, relu, kind, xin, torch.float32, acts)
            r32, e32 = rel_rms(y32, ref), elem(y32)
            assert e32 <= C_ELEM, (name, e32)
            for what, y in (("weights", layer_forward(conv, bn, relu, kind, xin, torch.float32, acts, weight_fn=bf16_drop_lo)),
                            ("input", layer_forward(conv, bn, relu, kind, bf16_drop_lo(xin), torch.float32, acts))):
                rr, ee = rel_rms(y, ref) / r32, elem(y)
                lines.append(f"{name:12s} {what:7s} rms ratio {rr:7.2f}  elementwise {ee:7.2f}")
                if not (rr > MARGIN * K_RMS or ee > MARGIN * C_ELEM):
                    weak.append((name, what, round(rr, 2), round(ee, 2)))
    print("\n" + "\n".join(lines))
    assert not weak, f"a dropped lo piece passes the EQTransformer layer bars (rms ratio, elementwise ratio): {weak}"


def _res_xa(net, B, seed):
    """the fp32 oracle's ResCNN output (eqt_mid4's input res.xa) for B synthetic windows"""
    seen = {}
    hook = net.bi_lstm_stack.register_forward_pre_hook(lambda mod, inp: seen.__setitem__("xa", inp[0].detach()))
    with torch.no_grad():
        net(OP.batch_pre(net, torch.from_numpy(synthetic_windows(B, net.in_samples, seed=seed))))
    hook.remove()
    return seen["xa"]


# LayerNorm's variance in one pass (E[z^2] - mean^2) is not caught, because at these inputs it is no fault: its error is
# (1 + mean^2 / var) ulps of the variance, and the transformers' LN inputs have |mean| below their deviation (LOG.md section 22)
MID_UNCAUGHT = ("ln_one_pass",)
MID_LOCAL = "step_rcp"  # one step of one direction, 2^-18 relative: inside today's chain bar K_MID, beyond the stage bars


def test_mid_faults_fail_the_stage_bars():
    """eqt_mid4's stages (tests/layer_f64.eqt_mid_stages) on the fp32 oracle's own values pass their bars; each planted fault of
    MID_FAULTS fails them by MARGIN, and the localized MID_LOCAL passes the chain check of test_gpu_layers_f64 (K_MID) while it
    fails the stage bars -- what the stage-by-stage check adds."""
    from tests.test_gpu_layers_f64 import K_MID

    net = load_pretrained("eqtransformer", "volpick")
    xa = _res_xa(net, 3, seed=3)
    rows = eqt_mid_stages(net, eqt_mid_acts(net, xa))
    assert not mid_bad(rows), mid_bad(rows)
    o64 = copy.deepcopy(net).double()
    ref, y32 = eqt_mid_chain(o64, xa.double()), eqt_mid_chain(net, xa)
    chain = lambda t: max(rel_rms(t[f"decoder{d}.in"], ref[d]) / rel_rms(y32[d], ref[d]) for d in range(3))
    lines, weak = [], []
    for fault in MID_FAULTS:
        t = eqt_mid_acts(net, xa, fault)
        rows = eqt_mid_stages(net, t)
        worst = max(rows, key=lambda r: max(r["rms_ratio"] / K_RMS, r["elem_ratio"] / C_ELEM) if r["finite"] else float("inf"))
        m = max(worst["rms_ratio"] / K_RMS, worst["elem_ratio"] / C_ELEM) if worst["finite"] else float("inf")
        ch = chain(t)
        lines.append(f"{fault:12s} worst stage {worst['name']:22s} {m:9.2f} x its bar   chain {ch:9.2f} x torch fp32")
        if fault in MID_UNCAUGHT:
            continue
        if not m > MARGIN:
            weak.append((fault, worst["name"], round(m, 2)))
        if fault == MID_LOCAL:
            assert ch <= K_MID, f"{fault}: the chain bar sees it already ({ch:.2f}): it shows nothing the stage bars add"
    print("\n" + "\n".join(lines))
    assert not weak, f"planted faults within {MARGIN} x the stage bars: {weak}"


def test_row_blocked_attention_is_the_oracle_module_bit_for_bit():
    """tests/layer_f64.attention_rows (the float64 reference of eqt_mid4 in blocks of query rows) is the oracle's module"""
    net = load_pretrained("eqtransformer", "volpick")
    x = torch.randn(2, 16, 300, generator=torch.Generator().manual_seed(5))
    for att in (net.transformer_d0.attention, net.transformer_d.attention, *net.pick_attentions):
        with torch.no_grad():
            for dtype in (torch.float32, torch.float64):
                a = att.to(dtype)
                assert torch.equal(a(x.to(dtype))[0], attention_rows(a, x.to(dtype), chunk=64))
                att.float()
