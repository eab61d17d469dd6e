"""Every layer of the shipped one-launch PhaseNet kernel (pn_window_kernel, bf16 three-piece operands) against float64, on the
kernel's own input to that layer (tests/layer_f64.py).  The kernel's DUMP instance (plan_flags[1] & 4) writes each layer's
fp32 output and the head's logits; its output probabilities must equal the shipped instance's bit for bit, which ties the
dumps to the shipped arithmetic.  EQTransformer's five conv kernels have DUMP instances under the same flag and are checked
the same way, every conv layer of the encoder, the ResCNN stack, the three decoders and the heads; its middle kernel (eqt_mid4)
is checked from its own input and output, which the default plan keeps in memory."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pipeline as OP
from oracle.models import load_pretrained
from tests.gpu_util import debug_tensors
from tests.layer_f64 import (C_ELEM, K_RMS, attention_form_plain, attention_weights, check_layer, eqt_layers, eqt_mid_chain,
                              eqt_mid_stages, mid_bad, phasenet_layers, rel_rms, report)
from tests.test_gpu_parity_wide import _as_array, _scaled_state
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd.synthetic import synthetic_windows

pytestmark = pytest.mark.gpu
DUMP = (0, 4)


def _rows(B):
    """Windows checked in float64: all of a batch of up to 16; of a large one the first, one in the middle and the last (one
    workgroup per window: the last is the last workgroup's)."""
    return None if B <= 16 else [0, B // 2, B - 2, B - 1]


def _run(weights, xn, state=None):
    """(probabilities of the shipped kernel, of the DUMP instance, the dumps)"""
    outs = []
    for flags in ((0,), DUMP):
        m = PhaseNet.from_pretrained(weights)
        if state is not None:
            m.load_state_dict(state)
        m._plan_flags = flags
        m._max_batch = max(256, xn.shape[0])
        m.cuda()
        try:
            outs.append(m(xn).cpu().numpy())
            if flags == DUMP:
                t = {k: torch.from_numpy(v) for k, v in debug_tensors(m, xn.shape[0]).items()}
        finally:
            m._release()
    return outs[0], outs[1], t


def _check(oracle, xn, weights, state=None, label=""):
    B = xn.shape[0]
    y, yd, t = _run(weights, xn, state)
    assert np.array_equal(y, yd, equal_nan=True), f"{label}: the DUMP instance's probabilities differ from the shipped kernel's"
    t["input"] = xn.float()
    rows = []
    for layer in phasenet_layers(oracle):
        rows.append(check_layer(layer, t, t[layer[0]], _rows(B)))
    print(f"\n[{label}] B={B}\n" + report(rows))
    bad = [r["name"] for r in rows if not (r["finite"] and r["rms_ratio"] <= K_RMS and r["elem_ratio"] <= C_ELEM)]
    assert not bad, f"{label}: layers beyond the float64 bars (rms ratio <= {K_RMS}, elementwise <= {C_ELEM}): {bad}"
    # the dumped logits are the probabilities' own: their softmax gives the shipped output back
    p = torch.softmax(t["logits"].double(), dim=1).numpy()
    assert np.abs(p - y).max() < 1e-6, label


@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
@pytest.mark.parametrize("B", [1, 7, 256])
def test_every_layer_matches_float64(weights, B):
    oracle = load_pretrained("phasenet", weights)
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(B, 3001, seed=900 + B)))
    _check(oracle, xn, weights, label=f"phasenet {weights}")


def _edge_windows(B, seed, T=3001):
    """energy at both ends of the window (the tiles that meet the zero padding) and a DC offset"""
    rng = np.random.default_rng(seed)
    x = synthetic_windows(B, T, seed=seed)
    t = np.arange(T)
    burst = np.exp(-((t[:, None] - np.array([40, T - 41])[None]) / 12.0) ** 2).sum(axis=1)
    x = x + (5.0 * x.std() * rng.standard_normal((B, 3, 1)) * np.sin(0.7 * t) * burst).astype(np.float32)
    x[B // 2:] += np.float32(3.0 * np.abs(x).max())  # DC offset
    return x.astype(np.float32)


@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
def test_edge_energy_and_dc_offset(weights):
    oracle = load_pretrained("phasenet", weights)
    x = _edge_windows(5, seed=931)
    # the network sees the windows without annotate_batch_pre's demeaning as well: the offset reaches the first layers
    xn = torch.cat([OP.batch_pre(oracle, torch.from_numpy(x)), torch.from_numpy(x / np.abs(x).max(axis=(1, 2), keepdims=True))])
    _check(oracle, xn, weights, label=f"phasenet {weights} edges + DC")


@pytest.mark.parametrize("scale", [1e20, 1e-20])
def test_activations_far_from_unity(scale):
    """test_gpu_parity_wide's scaling: down2.down's output (the first bf16-piece layer's input) at scale times its size"""
    oracle = load_pretrained("phasenet", "volpick")
    big = copy.deepcopy(oracle)
    big.load_state_dict(_scaled_state("phasenet", big.state_dict(), scale), strict=True)
    sd = PhaseNet.from_pretrained("volpick").state_dict()
    state = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _scaled_state("phasenet", sd, scale).items()}
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(3, 3001, seed=4500)))
    _check(big, xn, "volpick", state, label=f"phasenet activations x {scale:g}")


# ---- EQTransformer: eqt_mid4 from res.xa to decoder.in -------------------------------------------------------------------
K_MID = 4.0  # kernel relative RMS error of each decoder input <= K_MID x torch-fp32's from the same res.xa (LOG.md)


def _read(model, name, rows):
    """rows [0, rows) of the debug tensor `name` as the default plan left it; the tensor must be materialised (not LDS-only)"""
    lib, h = _lib.load(), model._handle
    for i in range(lib.vp_debug_tensor_count(h)):
        nm, c, l = C.c_char_p(), C.c_int(), C.c_int()
        _lib.check(lib.vp_debug_tensor_info(h, i, C.byref(nm), C.byref(c), C.byref(l)))
        if nm.value.decode() == name:
            a = np.empty((rows, c.value, l.value), np.float32)
            _lib.check(lib.vp_debug_tensor_read(h, i, rows, a.ctypes.data_as(C.c_void_p)))
            return torch.from_numpy(a)
    raise KeyError(name)


@pytest.mark.slow
@pytest.mark.parametrize("weights,B,rows", [("volpick", 1, [0]), ("volpick", 5, [0, 4]), ("volpick", 257, [0, 256]),
                                            ("volpick_95train", 5, [3])],
                         ids=["volpick-1", "volpick-5", "volpick-257", "volpick_95train-5"])
def test_eqt_middle_kernel_matches_float64(weights, B, rows):
    """B = 5 and 257 leave the last four-window workgroup of eqt_mid4 with one window; the checked rows include it."""
    oracle = load_pretrained("eqtransformer", weights)
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(B, 6000, seed=950 + B)))
    m = EQTransformer.from_pretrained(weights)
    m._max_batch = max(256, B)
    m.cuda()
    try:
        m(xn)
        xa = _read(m, "res.xa", B)[rows]
        dec = _read(m, "decoder.in", 3 * B)  # set-major: decoder d's window b at row d * B + b
    finally:
        m._release()
    o64 = copy.deepcopy(oracle).double()
    bad, lines = [], []
    for r, b in enumerate(rows):  # one window at a time: the attention's (T, T) blocks in float64
        ref = eqt_mid_chain(o64, xa[r:r + 1].double())
        y32 = eqt_mid_chain(oracle, xa[r:r + 1])
        for d, nm in enumerate(("decoder_d", "P branch", "S branch")):
            got = dec[d * B + b:d * B + b + 1]
            e, e32 = rel_rms(got, ref[d]), rel_rms(y32[d], ref[d])
            lines.append(f"window {b:3d} {nm:9s} rel rms {e:.2e} (torch fp32 {e32:.2e})  ratio {e / e32:5.2f}")
            if not (torch.isfinite(got).all() and e <= K_MID * e32):
                bad.append((b, nm, e / e32))
    print(f"\n[eqt_mid4 {weights}] B={B}\n" + "\n".join(lines))
    assert not bad, f"eqt_mid4 beyond {K_MID} x torch-fp32's error from res.xa: {bad}"


# ---- EQTransformer's five conv kernels (bf16 three-piece operands), layer by layer ----------------------------------------------
# front (encoder.0-2), enc36_b3 (encoder.3-6, res.act), res3t (the ResCNN's 14 convs), dec03 (decoder.0-3 of the three decoders),
# tail3 (decoder.4-6 and the heads' logits): their DUMP instances (plan_flags[1] & 4) write every conv's fp32 output.
SET_MAJOR = ("decoder.in", *(f"decoder.{k}" for k in range(7)), "logits")  # rows d B + b: decoder d's window b


def _halo_words(model):
    lib, bad, where = _lib.load(), C.c_int64(-1), C.c_char_p()
    _lib.check(lib.vp_debug_check_halos(model._handle, 0, C.byref(bad), C.byref(where)), "vp_debug_check_halos")
    return bad.value, where.value


def _eqt_dumps(model, B):
    """every tensor the DUMP plan keeps, under eqt_layers' names: the set-major ones split into decoder{d}.k / logits{d}"""
    t = {k: torch.from_numpy(v) for k, v in debug_tensors(model, B).items() if k not in SET_MAJOR}
    for name in SET_MAJOR:
        a = _read(model, name, 3 * B)
        for d in range(3):
            key = name.replace("decoder.", f"decoder{d}.") if name != "logits" else f"logits{d}"
            t[key] = a[d * B:(d + 1) * B]
    return t


def _eqt_run(xn, weights, state=None):
    """(probabilities of the shipped plan, of the DUMP plan, the dumps, the halo check) on xn; the DUMP plan runs a different
    batch of the same size first, so that a sample its dumps skip holds a stale value"""
    B = xn.shape[0]
    other = torch.flip(xn, dims=(0, 2)).contiguous()
    outs = []
    for flags in ((0,), DUMP):
        m = EQTransformer.from_pretrained(weights)
        if state is not None:
            m.load_state_dict(state)
        m._plan_flags = flags
        m._max_batch = max(256, B)
        m.cuda()
        try:
            if flags == DUMP:
                m(other)
            outs.append(_as_array(m(xn)))
            if flags == DUMP:
                t = _eqt_dumps(m, B)
                halos = _halo_words(m)
        finally:
            m._release()
    return outs[0], outs[1], t, halos


def _eqt_check(oracle, xn, weights, rows=None, state=None, label=""):
    """The shipped plan and the DUMP plan on xn (_eqt_run).  rows: windows checked in float64 (None = all)."""
    B = xn.shape[0]
    y, yd, t, halos = _eqt_run(xn, weights, state)
    assert np.array_equal(y, yd, equal_nan=True), f"{label}: the DUMP plan's probabilities differ from the shipped plan's"
    assert halos[0] == 0, f"{label}: the DUMP plan wrote into the zero margin of {halos[1]}"
    assert torch.equal(t["res.6.out"], t["res.xa"]), f"{label}: the dumped block-6 output is not the ResCNN kernel's output"
    # the dumped logits are the probabilities' own (sigmoid as v_exp + v_rcp in the kernel: 3e-7)
    for d in range(3):
        p = torch.sigmoid(t[f"logits{d}"][:, 0].double()).numpy()
        assert np.abs(p - y[:, d]).max() < 1e-6, (label, d)
    layers = eqt_layers(oracle)
    assert len(layers) == 7 + 1 + 3 * 7 + 3 * 8
    res = [check_layer(layer, t, t[layer[0]], rows) for layer in layers]
    print(f"\n[{label}] B={B} windows {'all' if rows is None else rows}\n" + report(res))
    # res.act is a BatchNorm without a conv (eqt_enc36_b3_kernel applies it as one fma): the elementwise bar only
    bad = [r["name"] for r in res
           if not (r["finite"] and r["elem_ratio"] <= C_ELEM and (r["name"] == "res.act" or r["rms_ratio"] <= K_RMS))]
    assert not bad, f"{label}: layers beyond the float64 bars (rms ratio <= {K_RMS}, elementwise <= {C_ELEM}): {bad}"


@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_eqt_conv_layers_match_float64(weights, B):
    """B = 1, 4 and 5 leave the ResCNN kernel's last workgroup (three windows) with a clamped, repeated window"""
    oracle = load_pretrained("eqtransformer", weights)
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(B, 6000, seed=960 + B)))
    _eqt_check(oracle, xn, weights, label=f"eqt {weights}")


@pytest.mark.slow
@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
def test_eqt_conv_layers_match_float64_257(weights):
    """B = 257: enc36_b3 and dec03 wrap their 256-workgroup grids (window 256 is workgroup 0's second), the ResCNN kernel's last
    workgroup holds windows 255, 256, 256, the tail's workgroups cross decoder changes; windows checked in all three decoders"""
    oracle = load_pretrained("eqtransformer", weights)
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(257, 6000, seed=977)))
    _eqt_check(oracle, xn, weights, rows=[0, 1, 128, 255, 256], label=f"eqt {weights}")


@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
def test_eqt_edge_energy_and_dc_offset(weights):
    oracle = load_pretrained("eqtransformer", weights)
    x = _edge_windows(5, seed=981, T=6000)
    xn = torch.cat([OP.batch_pre(oracle, torch.from_numpy(x)), torch.from_numpy(x / np.abs(x).max(axis=(1, 2), keepdims=True))])
    _eqt_check(oracle, xn, weights, label=f"eqt {weights} edges + DC")


@pytest.mark.parametrize("scale", [1e20, 1e-20])
def test_eqt_activations_far_from_unity(scale):
    """test_gpu_parity_wide's scaling: encoder stage 5's output and decoder stage 4's at scale times their size"""
    oracle = load_pretrained("eqtransformer", "volpick")
    big = copy.deepcopy(oracle)
    big.load_state_dict(_scaled_state("eqtransformer", big.state_dict(), scale), strict=True)
    sd = EQTransformer.from_pretrained("volpick").state_dict()
    state = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _scaled_state("eqtransformer", sd, scale).items()}
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(3, 6000, seed=4500)))
    _eqt_check(big, xn, "volpick", state=state, label=f"eqt activations x {scale:g}")


# ---- eqt_mid4 stage by stage (its DUMP instance), every window ------------------------------------------------------------
def _mid_check(oracle, xn, weights, state=None, label=""):
    """Every stage of every window of eqt_mid4 against float64 on the kernel's own input to it (tests/layer_f64.eqt_mid_stages).
    Returns the dumps."""
    B = xn.shape[0]
    y, yd, t, halos = _eqt_run(xn, weights, state)
    assert np.array_equal(y, yd, equal_nan=True), f"{label}: the DUMP plan's probabilities differ from the shipped plan's"
    assert halos[0] == 0, f"{label}: the DUMP plan wrote into the zero margin of {halos[1]}"
    # links: the stage inputs the float64 check starts from are what the kernel read (res.xa: the ResCNN kernel's output; the
    # block and transformer outputs: what eqt_mid4 wrote where the next stage reads it), and what the decoders read is the
    # dumped stage outputs -- decoder.in set 0 is transformer_d's LN2 output, sets 1 and 2 the pick branches' a.x
    assert torch.equal(t["res.6.out"], t["res.xa"]), label
    assert torch.equal(t["transformer_d"], t["decoder0.in"]), f"{label}: decoder.in set 0 is not transformer_d's dumped output"
    for k in range(2):
        assert t[f"pick_attentions.{k}.p"].shape == (B, 47, 47) and t[f"decoder{k + 1}.in"].shape == (B, 16, 47), label
    rows = eqt_mid_stages(oracle, t)
    print(f"\n[{label}] B={B}, every window\n" + report(rows))
    bad = mid_bad(rows)
    assert not bad, f"{label}: eqt_mid4 stages beyond the float64 bars (rms ratio <= {K_RMS}, elementwise <= {C_ELEM}): {bad}"
    return t


def _edited(weights, edits):
    """(oracle, state for the model) with the weights named in edits multiplied: {oracle parameter name: factor}"""
    oracle = copy.deepcopy(load_pretrained("eqtransformer", weights))
    params = dict(oracle.named_parameters())
    sd = EQTransformer.from_pretrained(weights).state_dict()
    with torch.no_grad():
        for n, f in edits.items():
            params[n].mul_(f)
            sd[n] = sd[n] * np.float32(f)
    return oracle, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in sd.items()}


@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
@pytest.mark.parametrize("B", [1, 4, 5])
def test_eqt_mid_stages_match_float64(weights, B):
    """B = 5 leaves the last four-window workgroup with one window (its team computes it, the clamped ones repeat it)"""
    oracle = load_pretrained("eqtransformer", weights)
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(B, 6000, seed=990 + B)))
    _mid_check(oracle, xn, weights, label=f"eqt_mid4 {weights}")


@pytest.mark.slow
@pytest.mark.parametrize("weights", ["volpick", "volpick_95train"])
def test_eqt_mid_stages_match_float64_257(weights):
    oracle = load_pretrained("eqtransformer", weights)
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(257, 6000, seed=997)))
    _mid_check(oracle, xn, weights, label=f"eqt_mid4 {weights}")


PLAIN = ("transformer_d.attention.Wx", "transformer_d.attention.Wt", "pick_attentions.1.Wx", "pick_attentions.1.Wt")


def test_eqt_mid_stages_plain_tanh_form():
    """test_gpu_eqt.test_attention_beyond_the_exp_product_guard's weights (projections x 40 in transformer_d and the S branch):
    every window past the |q|, |k| <= 30 guard, the plain tanh(q + k) form, which the probabilities alone checked before"""
    oracle, state = _edited("volpick", {n: 40.0 for n in PLAIN})
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(4, 6000, seed=991)))
    t = _mid_check(oracle, xn, "volpick", state, label="eqt_mid4 plain tanh")
    assert attention_form_plain(oracle.transformer_d.attention, t["transformer_d0"]).all()
    assert attention_form_plain(oracle.pick_attentions[1], t["pick_lstms.1.h"]).all()
    assert not attention_form_plain(oracle.transformer_d0.attention, t["bilstm.2"]).any()


def test_eqt_mid_stages_mixed_forms_in_one_workgroup():
    """transformer_d0's projections scaled until some windows of a four-window workgroup take the plain form and others the exp
    product (tests/test_gpu_round4.py's construction); which form each window took follows from float64 q and k"""
    B = 16
    x = synthetic_windows(B, 6000, seed=4242)
    x[1::4] *= 0.02  # quiet windows between loud ones: a spread of activation sizes at the attention input
    oracle = load_pretrained("eqtransformer", "volpick")
    xn = OP.batch_pre(oracle, torch.from_numpy(x))
    with torch.no_grad():
        xin = oracle.bi_lstm_stack(oracle.res_cnn_stack(oracle.encoder(xn)))
    att = oracle.transformer_d0.attention
    top = lambda w: torch.matmul(xin.permute(0, 2, 1), w.detach()).abs().amax(dim=(1, 2))
    scale = float(30.0 / torch.median(torch.maximum(top(att.Wt), top(att.Wx))))
    big, state = _edited("volpick", {"transformer_d0.attention.Wt": scale, "transformer_d0.attention.Wx": scale})
    t = _mid_check(big, xn, "volpick", state, label=f"eqt_mid4 mixed forms (x {scale:.2f})")
    plain = attention_form_plain(big.transformer_d0.attention, t["bilstm.2"]).reshape(-1, 4)
    assert (plain.any(dim=1) & ~plain.all(dim=1)).sum() >= 1, plain


@pytest.mark.parametrize("factor", [16.0, 1.0 / 16])
def test_eqt_mid_stages_saturated_and_near_zero_gates(factor):
    """the LSTM input weights of BiLSTM block 0 and of both pick LSTMs x 16 (gates saturated) and / 16 (near their midpoints)"""
    names = ["bi_lstm_stack.members.0.lstm.weight_ih_l0", "bi_lstm_stack.members.0.lstm.weight_ih_l0_reverse",
             "pick_lstms.0.weight_ih_l0", "pick_lstms.1.weight_ih_l0"]
    oracle, state = _edited("volpick", {n: factor for n in names})
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(4, 6000, seed=992)))
    _mid_check(oracle, xn, "volpick", state, label=f"eqt_mid4 LSTM input weights x {factor:g}")


def test_eqt_mid_stages_eps_dominated_pick_rows():
    """the P branch's Wa x 200: its band scores sit far below their rows' maxima, eps dominates the denominators (some weights
    underflow fp32: tests/layer_f64.P_FLOOR), edge rows t = 0 and 46 included"""
    oracle, state = _edited("volpick", {"pick_attentions.0.Wa": 200.0})
    xn = OP.batch_pre(oracle, torch.from_numpy(synthetic_windows(4, 6000, seed=993)))
    t = _mid_check(oracle, xn, "volpick", state, label="eqt_mid4 eps-dominated pick rows")
    att = oracle.pick_attentions[0]
    with torch.no_grad():
        _, e, _, _ = attention_weights(att, t["pick_lstms.0.h"], torch.float64)
        ex = torch.exp(e - e.max(dim=-1, keepdim=True).values)
    band = [(0, slice(0, 2)), (46, slice(45, 47))]
    sums = {i: ex[:, i, sl].sum(dim=-1) for i, sl in band}
    assert all(bool((s < att.eps).any()) for s in sums.values()), sums
    assert float((ex[:, 1:46].diagonal(offset=1, dim1=1, dim2=2) < att.eps).double().mean()) > 0.5
