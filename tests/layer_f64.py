"""Per-layer float64 check of a forward kernel's own arithmetic (tests/test_gpu_layers_f64.py, tests/test_layer_f64_cpu.py).

A layer's output, as a kernel computed it, is compared with the same layer computed in float64 ON THE KERNEL'S OWN INPUT to it
(the dump of the layer before, through the oracle's glue: crop, centred skip concat, padding).  An error upstream therefore
does not reach the layers behind it, and one layer's fault is not diluted by the softmax / sigmoid behind the network.

Two metrics per layer, both scaled by what fp32 arithmetic can do:
  * relative RMS error over the whole output, as a multiple of torch-fp32's relative RMS error on the same input
    (rms_ratio <= K_RMS): sees a lost piece product (fp32-grade bf16 three-piece operands keep the six of i + j <= 2);
  * elementwise |err| <= C_ELEM * 2^-24 * (sum |w| |x| + |b|), the sums in float64 (elem_ratio <= C_ELEM): sees a fault local to
    a tile, a lane group or a column, which the RMS dilutes.  ReLU and max-pool are 1-Lipschitz: post-activation values compare.
BatchNorm is applied unfolded, as the oracle runs it (eval mode); the kernels fold it into the weights, which the bound covers
(weights and bias of the bound are the folded ones, in float64).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import constants as OC

# Bars set from the measured MI355X numbers (LOG.md): the largest kernel / torch-fp32 RMS ratio was 2.88 (up0.same, a bf16-piece
# layer: the i + j = 3 products it drops are of the order of one fp32 product's rounding), the largest elementwise ratio 8.45
# (up2.same).  A dropped lo piece sits at 7-47x in RMS and 16-112x elementwise (tests/test_layer_f64_cpu.py).
K_RMS = 4.0    # kernel relative RMS error <= K_RMS x torch-fp32's on the same input
C_ELEM = 12.0  # |err| <= C_ELEM * 2^-24 * (sum |w||x| + |b|)
EPS24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# layers: (name, conv module, bn module or None, relu, kind, input builder); input builder(acts) -> fp32 tensor (B, C, L)
# acts: {tensor name: (B, C, L) float32 tensor} -- the kernel's dumps (GPU) or the oracle's own activations (CPU teeth test)
# ---------------------------------------------------------------------------------------------------------------------
def _centre(x, L):
    off = (x.shape[-1] - L) // 2
    return x[:, :, off:off + L]


def phasenet_layers(net):
    """Every PhaseNet layer under the names of the PhaseNet plan's debug tensors, in forward order."""
    m = dict(net.named_modules())
    out = [("inc", m["inc"], m["in_bn"], True, "conv", lambda a: a["input"])]
    for i in range(5):
        prev = "inc" if i == 0 else f"down{i - 1}.down"
        out.append((f"down{i}.same", m[f"down_branch.{i}.0"], m[f"down_branch.{i}.1"], True, "conv", lambda a, p=prev: a[p]))
        if i < 4:
            pad = (0, 0) if i == 0 else OC.PN_DOWN_PAD[i]
            out.append((f"down{i}.down", m[f"down_branch.{i}.2"], m[f"down_branch.{i}.3"], True, "conv",
                        lambda a, i=i, pad=pad: F.pad(a[f"down{i}.same"], pad)))
    for j in range(4):
        prev = "down4.same" if j == 0 else f"up{j - 1}.same"
        out.append((f"up{j}.convT", m[f"up_branch.{j}.0"], m[f"up_branch.{j}.1"], True, ("convT", 3 - j), lambda a, p=prev: a[p]))
        out.append((f"up{j}.same", m[f"up_branch.{j}.2"], m[f"up_branch.{j}.3"], True, "conv",
                    lambda a, j=j: torch.cat([a[f"down{3 - j}.same"], a[f"up{j}.convT"]], dim=1)))
    out.append(("logits", m["out"], None, False, "conv", lambda a: a["up3.same"]))
    return out


def phasenet_acts(net, x):
    """The fp32 oracle's activations under the debug tensors' names (CPU: the inputs of the teeth test)."""
    acts = {"input": x}
    with torch.no_grad():
        for name, conv, bn, relu, kind, inp in phasenet_layers(net):
            acts[name] = layer_forward(conv, bn, relu, kind, inp(acts), torch.float32, acts)
    return acts


# ---------------------------------------------------------------------------------------------------------------------
EQT_DECODERS = ("decoder_d", "pick_decoders.0", "pick_decoders.1")
EQT_HEADS = ("conv_d", "pick_convs.0", "pick_convs.1")


def _eqt_act0(bn, x):
    """relu(bn(x)) in float64, rounded to fp32: the input of a ResCNN block's conv1 (the kernels apply the BatchNorm as one fma)"""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return torch.relu(x.double() * s.reshape(-1, 1) + b.reshape(-1, 1)).float()


def eqt_layers(net):
    """Every EQTransformer conv layer in forward order, under the names of the debug tensors of plan_flags[1] & 4 (decoder d's
    stage k: "decoder{d}.{k}", its input "decoder{d}.in", its head's logits "logits{d}": one set of the set-major tensors).
    Kinds beyond phasenet_layers': ("pool",) conv + ReLU, then max-pool(2) with the odd tail padded as the encoder does;
    ("res", x) the ResCNN block output x + conv2(mid); "bn" relu(norm1_0(encoder.6)), res.act, no conv (elementwise bar only)."""
    m = dict(net.named_modules())
    out = []
    for k in range(7):
        prev = "input" if k == 0 else f"encoder.{k - 1}"
        out.append((f"encoder.{k}", m[f"encoder.convs.{k}"], None, True, ("pool",), lambda a, p=prev: a[p]))
    out.append(("res.act", None, m["res_cnn_stack.members.0.norm1"], True, "bn", lambda a: a["encoder.6"]))
    for i in range(7):
        blk = m[f"res_cnn_stack.members.{i}"]
        pad = (0, 1) if blk.right_pad else (0, 0)  # K = 2: TF "same" pads on the right only
        prev = "encoder.6" if i == 0 else f"res.{i - 1}.out"
        # block 0 reads res.act, which is in memory (written behind encoder stage 6); the later blocks' conv1 inputs exist in
        # the ResCNN kernel's LDS only and are recomputed from the block before's output
        act = (lambda a: a["res.act"]) if i == 0 else (lambda a, p=prev, bn=blk.norm1: _eqt_act0(bn, a[p]))
        out.append((f"res.{i}.mid", blk.conv1, blk.norm2, True, "conv", lambda a, act=act, pad=pad: F.pad(act(a), pad)))
        out.append((f"res.{i}.conv2", blk.conv2, None, False, "conv", lambda a, i=i, pad=pad: F.pad(a[f"res.{i}.mid"], pad)))
        out.append((f"res.{i}.out", blk.conv2, None, False, ("res", prev), lambda a, i=i, pad=pad: F.pad(a[f"res.{i}.mid"], pad)))
    for d, dec in enumerate(EQT_DECODERS):
        for k in range(7):
            prev = f"decoder{d}.in" if k == 0 else f"decoder{d}.{k - 1}"
            crop = k in m[dec].crops  # stage 2: 375 = 2 x 188 - 1

            def up(a, p=prev, crop=crop):
                x = F.interpolate(a[p], scale_factor=2, mode="nearest")
                return x[:, :, :-1] if crop else x
            out.append((f"decoder{d}.{k}", m[f"{dec}.convs.{k}"], None, True, "conv", up))
        out.append((f"logits{d}", m[EQT_HEADS[d]], None, False, "conv", lambda a, d=d: a[f"decoder{d}.6"]))
    return out


def eqt_acts(net, x):
    """The fp32 oracle's activations under eqt_layers' names (CPU: the inputs of the teeth test); the middle (BiLSTM stack,
    transformers, pick branches) is the oracle's own, from res.6.out."""
    acts = {"input": x}
    with torch.no_grad():
        for name, conv, bn, relu, kind, inp in eqt_layers(net):
            if name == "decoder0.0":
                for d, h in enumerate(eqt_mid_chain(net, acts["res.6.out"])):
                    acts[f"decoder{d}.in"] = h
            acts[name] = layer_forward(conv, bn, relu, kind, inp(acts), torch.float32, acts)
    return acts


# ---------------------------------------------------------------------------------------------------------------------
def _folded(conv, bn, dtype):
    """(weight, bias) with BatchNorm folded in, float64 -> dtype; weight laid out as the module's."""
    w = conv.weight.detach().double()
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(w.shape[1 if isinstance(conv, torch.nn.ConvTranspose1d) else 0], dtype=torch.float64)
    if bn is not None:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shape = (1, -1, 1) if isinstance(conv, torch.nn.ConvTranspose1d) else (-1, 1, 1)
        w = w * s.reshape(shape)
        b = (b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return w.to(dtype), b.to(dtype)


def _conv(conv, x, w, b, kind):
    if kind == "conv":
        return F.conv1d(x, w, b, stride=conv.stride, padding=conv.padding, dilation=conv.dilation)
    return F.conv_transpose1d(x, w, b, stride=conv.stride, padding=conv.padding)


def _glue_out(y, kind, acts):
    if isinstance(kind, tuple) and kind[0] == "pool":  # EQTransformer encoder: TF "same" max-pool on odd lengths
        if y.shape[-1] % 2:
            y = F.pad(y, (0, 1), "constant", OC.EQT_POOL_PAD_VALUE)
        return F.max_pool1d(y, 2)
    if isinstance(kind, tuple) and kind[0] == "res":
        return y
    if isinstance(kind, tuple):  # PhaseNet transposed conv: crop, then centre on the skip tensor it is concatenated with
        y = y[:, :, OC.PN_UP_CROP[0]:y.shape[-1] - OC.PN_UP_CROP[1]]
        return _centre(y, acts[f"down{kind[1]}.same"].shape[-1]) if acts is not None else y
    return y


def layer_forward(conv, bn, relu, kind, x, dtype, acts=None, weight_fn=None):
    """The layer as the oracle runs it (conv, BatchNorm unfolded, ReLU) in `dtype`; weight_fn(w) may alter the conv weight
    (teeth test).  acts: for the centring of a transposed conv's output (PhaseNet) and the residual stream a ResCNN block's
    output adds to (EQTransformer)."""
    if kind == "bn":
        y = x.to(dtype)
    else:
        ck = "convT" if kind == "convT" or (isinstance(kind, tuple) and kind[0] == "convT") else "conv"
        w = conv.weight.detach().to(dtype)
        if weight_fn is not None:
            w = weight_fn(w)
        b = conv.bias.detach().to(dtype) if conv.bias is not None else None
        y = _conv(conv, x.to(dtype), w, b, ck)
    if isinstance(kind, tuple) and kind[0] == "res":
        y = acts[kind[1]].to(dtype) + y
    if bn is not None:
        y = F.batch_norm(y, bn.running_mean.to(dtype), bn.running_var.to(dtype), bn.weight.detach().to(dtype),
                         bn.bias.detach().to(dtype), False, 0.0, bn.eps)
    if relu:
        y = torch.relu(y)
    return _glue_out(y, kind, acts)


def elem_scale(conv, bn, kind, x, acts=None):
    """sum |w_folded| |x| + |b_folded| per output element, float64."""
    if kind == "bn":  # |s x| + |b|: the BatchNorm as one fma
        sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        sh = bn.bias.detach().double() - bn.running_mean.detach().double() * sc
        return x.double().abs() * sc.abs().reshape(-1, 1) + sh.abs().reshape(-1, 1)
    ck = "convT" if kind == "convT" or (isinstance(kind, tuple) and kind[0] == "convT") else "conv"
    w, b = _folded(conv, bn, torch.float64)
    s = _conv(conv, x.double().abs(), w.abs(), b.abs(), ck)
    if isinstance(kind, tuple) and kind[0] == "res":  # the residual add: |x_prev| joins the bound
        s = s + acts[kind[1]].double().abs()
    return _glue_out(s, kind, acts)


def bf16_drop_lo(t):
    """t truncated to its first two bf16 pieces (hi + mid): the lo piece of the three-piece split dropped."""
    t32 = t.float()
    hi = t32.to(torch.bfloat16).float()
    mid = (t32 - hi).to(torch.bfloat16).float()
    return (hi + mid).to(t.dtype)


def rel_rms(got, ref):
    return float(torch.sqrt(torch.mean((got.double() - ref) ** 2)) / max(float(torch.sqrt(torch.mean(ref ** 2))), 1e-300))


def check_layer(layer, acts, got, rows=None):
    """Metrics of one layer.  got: the kernel's output (B, C, L); rows: windows to check (None = all).
    Returns dict(name, rms, rms32, rms_ratio, elem_ratio, elem32_ratio)."""
    name, conv, bn, relu, kind, inp = layer
    sub = {k: (v if rows is None else v[rows]) for k, v in acts.items()}
    x = inp(sub).float()
    got = (got if rows is None else got[rows]).double()
    with torch.no_grad():
        ref = layer_forward(conv, bn, relu, kind, x, torch.float64, sub)
        y32 = layer_forward(conv, bn, relu, kind, x, torch.float32, sub)
        scale = EPS24 * elem_scale(conv, bn, kind, x, sub)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    floor = EPS24 * float(scale.max()) * 1e-6  # (all-zero rows: nothing to measure against)
    rms, rms32 = rel_rms(got, ref), rel_rms(y32, ref)
    return dict(name=name, rms=rms, rms32=rms32, rms_ratio=rms / max(rms32, 1e-300),
                elem_ratio=float(((got - ref).abs() / (scale + floor)).max()),
                elem32_ratio=float(((y32.double() - ref).abs() / (scale + floor)).max()),
                finite=bool(torch.isfinite(got).all()))


def report(rows):
    return "\n".join(f"{r['name']:12s} rel rms {r['rms']:.2e} (torch fp32 {r['rms32']:.2e})  ratio {r['rms_ratio']:5.2f}   "
                     f"elementwise {r['elem_ratio']:5.2f} x 2^-24 sum|w||x| (fp32 {r['elem32_ratio']:5.2f})" for r in rows)


# ---------------------------------------------------------------------------------------------------------------------
# EQTransformer's middle (eqt_mid4: BiLSTM stack, two transformers, the P / S branches' LSTM + banded attention), from its
# input res.xa to its output decoder.in, as one chain: fp32 VALU arithmetic with LSTM recurrences, exp and layer norms, so one
# RMS bar per decoder input, calibrated on torch-fp32 like the conv layers.
# ---------------------------------------------------------------------------------------------------------------------
def attention_rows(att, x, chunk=500):
    """oracle.models._SeqSelfAttention.forward(x)[0] evaluated in blocks of query rows (the full form holds a (B, T, T, units)
    tensor: 9 GB per EQTransformer window in float64).  Every reduction is the module's, over the same axis in the same
    order, so the result is the module's bit for bit (tests/test_layer_f64_cpu.py)."""
    x = x.permute(0, 2, 1)  # (B, T, C)
    T = x.shape[1]
    k = torch.matmul(x, att.Wx).unsqueeze(1)
    out = []
    for t0 in range(0, T, chunk):
        q = torch.matmul(x[:, t0:t0 + chunk], att.Wt).unsqueeze(2)
        h = torch.tanh(q + k + att.bh)
        e = (torch.matmul(h, att.Wa) + att.ba).squeeze(-1)
        e = torch.exp(e - e.max(dim=-1, keepdim=True).values)
        if att.attention_width is not None:
            lower = torch.arange(T) - att.attention_width // 2
            idx = torch.arange(t0, t0 + e.shape[1]).unsqueeze(1)
            e = torch.where(torch.logical_and(lower <= idx, idx < lower + att.attention_width), e, torch.zeros_like(e))
        a = e / (e.sum(dim=-1, keepdim=True) + att.eps)
        out.append(torch.matmul(a, x))
    return torch.cat(out, dim=1).permute(0, 2, 1)


def eqt_mid_chain(net, x):
    """decoder.in's three sets (decoder_d's input, the P and S branches' attention outputs) from res.xa, in net's dtype."""
    with torch.no_grad():
        h = net.bi_lstm_stack(x)
        for tr in (net.transformer_d0, net.transformer_d):
            y = tr.norm1(h + attention_rows(tr.attention, h))
            h = tr.norm2(y + tr.ff(y))
        outs = [h]
        for lstm, att in zip(net.pick_lstms, net.pick_attentions):
            px = lstm(h.permute(2, 0, 1))[0].permute(1, 2, 0)
            outs.append(attention_rows(att, px))
    return outs
