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


# ---------------------------------------------------------------------------------------------------------------------
# eqt_mid4 stage by stage.  Its DUMP instance (plan_flags[1] & 4) writes every stage's fp32 values; each stage is computed in
# float64 and in torch fp32 from the kernel's OWN dumped input to it (teacher forcing: LSTM step t from the dumped x_t, h_{t-1},
# c_{t-1}), so an error is charged to the stage that made it, and the 47 steps of a recurrence are checked independently.
# Two bars per stage, as for the convs: relative RMS error <= K_RMS x torch-fp32's on the same input (at least RMS_FLOOR), and
# |err| <= C_ELEM * 2^-24 * scale elementwise, where scale is the stage's sum |w||x| + |b| carried to its output through the
# stage's derivatives.  Terms of scale that stand for a fixed number of ulps enter divided by C_ELEM, so that they count once.
# ---------------------------------------------------------------------------------------------------------------------
ACT_ULP = 8.0  # v_exp_f32 and v_rcp_f32 are 1 ulp each: a gate's sigmoid rcp(1 + exp2) is within 3 ulps of [0, 1], tanh as
               # 2 sigmoid(2x) - 1 within 6; a softmax weight exp * rcp within 3 ulps relative
SUM_ULP = 46.0  # a sum of 47 terms in any order: within 46 ulps of the sum of magnitudes (the softmax denominator)
RMS_FLOOR = 2.0 ** -25  # floor of torch-fp32's relative RMS error, half an ulp: one rounding (where fp32 is exact)
# Absolute floor of the attention weights.  A band score so far below its row's maximum that exp(e - max) falls under the
# smallest normal fp32 keeps none of its digits (v_exp_f32 flushes it to zero, torch keeps a subnormal), so no relative bound
# holds for its p = ex / (sum + eps); every such p is below 2^-126 / eps = 1.2e-33.
P_FLOOR = 2.0 ** -126 / OC.EQT_ATTENTION_EPS
EQT_TRANSFORMERS = ("transformer_d0", "transformer_d")


def _metrics(name, got, ref, y32, scale, form=None):
    """check_layer's row for a stage: got (kernel), ref (float64), y32 (torch fp32), scale (the elementwise bar / (C_ELEM 2^-24)).
    form: the absolute error, in ulps of 1, that the kernel's activation form makes whatever its argument (None: none); the RMS
    bar is then K_RMS x the larger of torch-fp32's relative RMS error and this one's."""
    got, y32 = got.double(), y32.double()
    den = EPS24 * scale.double() + 1e-300
    rms, rms32 = rel_rms(got, ref), rel_rms(y32, ref)
    if form is not None:
        rms32 = max(rms32, rel_rms(ref + EPS24 * form, ref))
    return dict(name=name, rms=rms, rms32=rms32, rms_ratio=rms / max(rms32, RMS_FLOOR),
                elem_ratio=float(((got - ref).abs() / den).max()), elem32_ratio=float(((y32 - ref).abs() / den).max()),
                finite=bool(torch.isfinite(got).all()))


def _prev(v, reverse):
    """the state step t reads: v at t - 1 (t + 1 backward), zero before a direction's first step"""
    z = torch.zeros_like(v[..., :1])
    return torch.cat([v[..., 1:], z], -1) if reverse else torch.cat([z, v[..., :-1]], -1)


def _lstm_w(mod, sfx):
    """(W_ih, W_hh, b_ih + b_hh) of one direction of an nn.LSTM (sfx "" or "_reverse"), as stored"""
    g = lambda n: getattr(mod, f"{n}_l0{sfx}").detach()
    return g("weight_ih"), g("weight_hh"), g("bias_ih") + g("bias_hh")


def lstm_step(w, x, hp, cp, dtype):
    """every step t of one LSTM direction at once from x_t, h_{t-1}, c_{t-1} (B, C, T), in dtype: ((i, f, g, o), c_t, h_t)"""
    w_ih, w_hh, b = (v.to(dtype) for v in w)
    z = (torch.einsum("gc,bct->bgt", w_ih, x.to(dtype)) + torch.einsum("gu,but->bgt", w_hh, hp.to(dtype))
         + b.reshape(1, -1, 1))
    i, f, g, o = z.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * cp.to(dtype) + i * g
    return (i, f, g, o), c, o * torch.tanh(c)


def check_lstm(name, w, x, h, c, reverse):
    """rows name.c, name.h: one direction, teacher-forced.  w: _lstm_w; x: the stage's input; h, c: the kernel's (B, 16, T)."""
    hp, cp = _prev(h, reverse), _prev(c, reverse)
    (i, f, g, o), c64, h64 = lstm_step(w, x, hp, cp, torch.float64)
    _, c32, h32 = lstm_step(w, x, hp, cp, torch.float32)
    # the gates' pre-activations are within C_ELEM 2^-24 S (S = sum |W_ih||x| + sum |W_hh||h| + |b|); first order through the step,
    # plus ACT_ULP ulps per activation and the roundings of c = f c + i g (two) and of h = o tanh(c) (two, and the product c 2 log2 e
    # that feeds v_exp_f32: tanh'(c) |c| four ulps)
    w_ih, w_hh, b = (v.double().abs() for v in w)
    S = (torch.einsum("gc,bct->bgt", w_ih, x.double().abs()) + torch.einsum("gu,but->bgt", w_hh, hp.double().abs())
         + b.reshape(1, -1, 1))
    Si, Sf, Sg, So = S.chunk(4, dim=1)
    a = ACT_ULP / C_ELEM
    di, df, do, dg = i * (1 - i) * Si + a, f * (1 - f) * Sf + a, o * (1 - o) * So + a, (1 - g * g) * Sg + a
    cpd = cp.double()
    dc = cpd.abs() * df + g.abs() * di + i * dg + 2.0 / C_ELEM * ((f * cpd).abs() + (i * g).abs())
    tc = torch.tanh(c64)
    dh = tc.abs() * do + o * ((1 - tc * tc) * (dc + 4.0 / C_ELEM * c64.abs()) + a) + 2.0 / C_ELEM * h64.abs()
    # the kernel's tanh is 2 sigmoid(2x) - 1 = 1 - 2 rcp(exp2(2x log2 e) + 1): v_exp_f32 and v_rcp_f32 leave one ulp of 1 each,
    # absolute, also where tanh(x) ~ x is small (near-zero gates, small cell states): g's error enters c with i, tanh(c)'s h with o
    form_c = 2.0 * i
    form_h = o * (2.0 + (1 - tc * tc) * form_c)
    return [_metrics(name + ".c", c, c64, c32, dc, form_c), _metrics(name + ".h", h, h64, h32, dh, form_h)]


def check_linear(name, conv, bn, relu, x, got):
    """a Conv1d(k = 1) / Linear stage (+ BatchNorm, + ReLU) on its dumped input, with the conv layers' elementwise scale"""
    with torch.no_grad():
        ref = layer_forward(conv, bn, relu, "conv", x.float(), torch.float64)
        y32 = layer_forward(conv, bn, relu, "conv", x.float(), torch.float32)
        return _metrics(name, got, ref, y32, elem_scale(conv, bn, "conv", x))


def _conv1x1(lin):
    """nn.Linear as the Conv1d(k = 1) it is along the time axis (layer_forward and elem_scale take conv modules)"""
    conv = torch.nn.Conv1d(lin.in_features, lin.out_features, 1)
    with torch.no_grad():
        conv.weight.copy_(lin.weight.detach().unsqueeze(-1))
        conv.bias.copy_(lin.bias.detach())
    return conv


def _band(T, width):
    """the module's band mask [i][j]: lower_j <= i < lower_j + width, lower_j = j - width // 2"""
    t = torch.arange(T)
    lower = t - width // 2
    idx = t.unsqueeze(1)
    return torch.logical_and(lower <= idx, idx < lower + width)


def attention_weights(att, x, dtype):
    """(p, e, q, k) of the module on x (B, C, T) in dtype: p (B, T, T) by its rule (max over the full row, the band mask, eps)"""
    W = lambda v: v.detach().to(dtype)
    xt = x.to(dtype).permute(0, 2, 1)
    q, k = torch.matmul(xt, W(att.Wt)), torch.matmul(xt, W(att.Wx)) + W(att.bh)
    e = (torch.matmul(torch.tanh(q.unsqueeze(2) + k.unsqueeze(1)), W(att.Wa)) + W(att.ba)).squeeze(-1)
    ex = torch.exp(e - e.max(dim=-1, keepdim=True).values)
    if att.attention_width is not None:
        ex = torch.where(_band(e.shape[-1], att.attention_width), ex, torch.zeros_like(ex))
    return ex / (ex.sum(dim=-1, keepdim=True) + att.eps), e, q, k


def attention_form_plain(att, x):
    """per window: does eqt_mid4 take the plain tanh form (some |q|, |k| beyond 30, from float64 q and k) or the exp product"""
    xt = x.double().permute(0, 2, 1)
    q = torch.matmul(xt, att.Wt.detach().double())
    k = torch.matmul(xt, att.Wx.detach().double()) + att.bh.detach().double()
    return torch.maximum(q.abs().amax(dim=(1, 2)), k.abs().amax(dim=(1, 2))) > 30.0


def check_attention(name, att, x, p, ax):
    """rows name.p (from the dumped input), name.ax (a.x against the kernel's own p) and name.ax64 (a.x against float64 end to end).
    x: the dumped input (B, 16, T); p: the kernel's weights (B, T, T); ax: its a.x (B, 16, T), before any residual."""
    with torch.no_grad():
        p64, e, q, k = attention_weights(att, x, torch.float64)
        p32 = attention_weights(att, x, torch.float32)[0]
        # score error: C_ELEM 2^-24 sum_u |Wa_u| (sum_c |x_ic||Wt_cu| + sum_c |x_jc||Wx_cu| + |bh_u| + 1) -- the rounded projections
        # move tanh's argument (the exp-product form's exp(2q) exp(2k) by as much, relative), the 1 the activation's own error
        xa = x.double().abs().permute(0, 2, 1)
        qa = torch.matmul(xa, att.Wt.detach().double().abs())
        ka = torch.matmul(xa, att.Wx.detach().double().abs()) + att.bh.detach().double().abs()
        wa = att.Wa.detach().double().abs().squeeze(-1)
        sc = (torch.matmul(qa, wa).unsqueeze(2) + torch.matmul(ka, wa).unsqueeze(1) + wa.sum())
        # p_ij = ex_ij / (sum + eps): |d ln p_ij| <= |d x_ij| + sum_l p_il |d x_il| with x = e - max, each within twice the row's
        # largest score error; the argument rounding of exp: 2 |x| per term, ACT_ULP for exp and rcp, SUM_ULP for the sum
        band = _band(e.shape[-1], att.attention_width) if att.attention_width is not None else torch.ones_like(p64, dtype=torch.bool)
        xm = torch.where(band, (e - e.max(dim=-1, keepdim=True).values).abs(), torch.zeros_like(e)).amax(dim=-1, keepdim=True)
        ps = p64 * (4.0 * sc.amax(dim=-1, keepdim=True) + (ACT_ULP + SUM_ULP + 4.0 * xm) / C_ELEM) + P_FLOOR / (C_ELEM * EPS24)
        rows = [_metrics(name + ".p", p, p64, p32, ps)]
        xd = x.double()
        mm = lambda a, b: torch.einsum("bij,bcj->bci", a, b)
        rows.append(_metrics(name + ".ax", ax, mm(p.double(), xd), mm(p.float(), x.float()), mm(p.double().abs(), xd.abs())))
        rows.append(_metrics(name + ".ax64", ax, mm(p64, xd), mm(p32, x.float()), mm(p64.abs(), xd.abs()) + mm(ps, xd.abs())))
    return rows


def check_ln(name, ln, x, y, got):
    """LayerNormalization of x + y (both the kernel's fp32 values; the sum in float64).  The kernel's fp32 sum, mean and
    deviations are within a few ulps of Z = |x| + |y| and of its channel mean / max; what they move is carried by 1 / sigma,
    into the deviations and, through the variance, into the scale: the bar grows with mean / sigma (the conditioning)."""
    with torch.no_grad():
        gam, bet = ln.gamma.detach().double().reshape(1, -1, 1), ln.beta.detach().double().reshape(1, -1, 1)
        z = x.double() + y.double()
        d = z - z.mean(dim=1, keepdim=True)
        sd = torch.sqrt((d * d).mean(dim=1, keepdim=True) + ln.eps)
        ref = d / sd * gam + bet
        y32 = ln.float()(x.float() + y.float())
        Z = x.double().abs() + y.double().abs()
        zm, zx = Z.mean(dim=1, keepdim=True), Z.amax(dim=1, keepdim=True)
        scale = gam.abs() * ((Z + zm) / sd + d.abs() / sd * ((zx + zm) / sd + 1)) + bet.abs()
        return _metrics(name, got, ref, y32, scale)


def eqt_mid_stages(net, t):
    """Every stage of eqt_mid4 against float64 on the kernel's own input to it.  t: {debug tensor name: (B, C, T)} -- the DUMP
    instance's (GPU) or eqt_mid_acts' (CPU teeth test), decoder{1,2}.in the P / S branches' attention outputs.  One row per stage
    (check_layer's keys), in forward order."""
    rows, x = [], t["res.xa"]
    for i, blk in enumerate(net.bi_lstm_stack.members):
        h, c = t[f"bilstm.{i}.h"], t[f"bilstm.{i}.c"]
        for dr, sfx in enumerate(("", "_reverse")):
            rows += check_lstm(f"bilstm.{i}.{'fb'[dr]}", _lstm_w(blk.lstm, sfx), x, h[:, 16 * dr:16 * dr + 16],
                               c[:, 16 * dr:16 * dr + 16], dr == 1)
        rows.append(check_linear(f"bilstm.{i}", blk.conv, blk.norm, False, h, t[f"bilstm.{i}"]))
        x = t[f"bilstm.{i}"]
    for name in EQT_TRANSFORMERS:
        tr = getattr(net, name)
        rows += check_attention(name, tr.attention, x, t[f"{name}.p"], t[f"{name}.att"])
        rows.append(check_ln(f"{name}.y1", tr.norm1, x, t[f"{name}.att"], t[f"{name}.y1"]))
        rows.append(check_linear(f"{name}.ff1", _conv1x1(tr.ff.lin1), None, True, t[f"{name}.y1"], t[f"{name}.ff1"]))
        rows.append(check_linear(f"{name}.ff2", _conv1x1(tr.ff.lin2), None, False, t[f"{name}.ff1"], t[f"{name}.ff2"]))
        rows.append(check_ln(name, tr.norm2, t[f"{name}.y1"], t[f"{name}.ff2"], t[name]))
        x = t[name]
    for k, (lstm, att) in enumerate(zip(net.pick_lstms, net.pick_attentions)):
        h = t[f"pick_lstms.{k}.h"]
        rows += check_lstm(f"pick_lstms.{k}", _lstm_w(lstm, ""), x, h, t[f"pick_lstms.{k}.c"], False)
        rows += check_attention(f"pick_attentions.{k}", att, h, t[f"pick_attentions.{k}.p"], t[f"decoder{k + 1}.in"])
    return rows


def mid_bad(rows):
    """the rows beyond the bars"""
    return [r["name"] for r in rows if not (r["finite"] and r["rms_ratio"] <= K_RMS and r["elem_ratio"] <= C_ELEM)]


# ---- the CPU teeth test's emulation of the DUMP instance, with one planted fault ------------------------------------------
MID_FAULTS = {
    "rcp": "bilstm block 0: every gate activation to 11 significant bits (a reciprocal or exp of 2^-12 relative error)",
    "gnext": "pick_lstms.0: the last step reads the input projection of the step before (the clamped re-read)",
    "step_rcp": "pick_lstms.0: the last step's gate activations to 17 significant bits (2^-18 relative)",
    "band_edge": "pick_attentions.0: row 46's denominator counts the padding column 47",
    "ln_one_pass": "transformer_d0's LN1: the variance as E[z^2] - mean^2 in fp32",
    "no_eps": "pick_attentions.0: the softmax without eps",
    "exp_factor": "transformer_d0's scores in the exp-product form, exp(2q) to 11 significant bits",
}


def _round_bits(v, bits):
    m, e = torch.frexp(v)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def _lstm_run(w, x, reverse, fault=None):
    """one LSTM direction over the window, step by step in fp32 as the kernel runs it: (h, c) (B, 16, T)"""
    w_ih, w_hh, b = w
    B, _, T = x.shape
    gx = torch.einsum("gc,bct->bgt", w_ih, x) + b.reshape(1, -1, 1)
    h, c = x.new_zeros(B, 16), x.new_zeros(B, 16)
    H, Cs = x.new_zeros(B, 16, T), x.new_zeros(B, 16, T)
    order = list(range(T - 1, -1, -1)) if reverse else list(range(T))
    for s, t in enumerate(order):
        bits = 11 if fault == "rcp" else 17 if fault == "step_rcp" and s == T - 1 else None
        sig = (lambda v: _round_bits(torch.sigmoid(v), bits)) if bits else torch.sigmoid
        i, f, g, o = (gx[..., order[s - 1] if fault == "gnext" and s == T - 1 else t] + h @ w_hh.T).chunk(4, dim=1)
        g = 2 * sig(2 * g) - 1 if bits else torch.tanh(g)
        c = sig(f) * c + sig(i) * g
        h = sig(o) * torch.tanh(c)
        H[..., t], Cs[..., t] = h, c
    return H, Cs


def _attention_emul(att, x, fault=None):
    """(p, a.x) of the module on x (B, C, T) in fp32, with the faults of MID_FAULTS that concern an attention"""
    xt = x.permute(0, 2, 1)
    q, k = xt @ att.Wt, xt @ att.Wx + att.bh
    if fault == "exp_factor":  # tanh(q + k) = 1 - 2 / (exp(2q) exp(2k) + 1)
        th = 1 - 2 / (_round_bits(torch.exp(2 * q), 11).unsqueeze(2) * torch.exp(2 * k).unsqueeze(1) + 1)
    else:
        th = torch.tanh(q.unsqueeze(2) + k.unsqueeze(1))
    e = (th @ att.Wa).squeeze(-1) + att.ba
    m = e.max(dim=-1, keepdim=True).values
    ex = torch.exp(e - m)
    T = e.shape[-1]
    if att.attention_width is not None:
        ex = torch.where(_band(T, att.attention_width), ex, torch.zeros_like(ex))
    den = ex.sum(dim=-1, keepdim=True)
    if fault == "band_edge":  # column 47's score from the zero padding column (k = bh)
        e47 = torch.tanh(q[:, T - 1] + att.bh) @ att.Wa + att.ba
        den = den.clone()
        den[:, T - 1] += torch.exp(e47 - m[:, T - 1])
    p = ex / (den + (0.0 if fault == "no_eps" else att.eps))
    return p, torch.einsum("bij,bcj->bci", p, x)


def _ln_emul(ln, z, fault=None):
    if fault != "ln_one_pass":
        return ln(z)
    mean = z.mean(dim=1, keepdim=True)
    var = (z * z).mean(dim=1, keepdim=True) - mean * mean + ln.eps
    return (z - mean) / torch.sqrt(var) * ln.gamma + ln.beta


def eqt_mid_acts(net, xa, fault=None):
    """eqt_mid4's dumps (eqt_mid_stages' names) as the fp32 oracle computes them from res.xa, free running, with one fault of
    MID_FAULTS planted (None: none)"""
    t = {"res.xa": xa}
    with torch.no_grad():
        x = xa
        for i, blk in enumerate(net.bi_lstm_stack.members):
            f = fault if i == 0 and fault == "rcp" else None
            hc = [_lstm_run(_lstm_w(blk.lstm, sfx), x, sfx != "", f) for sfx in ("", "_reverse")]
            t[f"bilstm.{i}.h"] = torch.cat([hc[0][0], hc[1][0]], dim=1)
            t[f"bilstm.{i}.c"] = torch.cat([hc[0][1], hc[1][1]], dim=1)
            x = t[f"bilstm.{i}"] = blk.norm(blk.conv(t[f"bilstm.{i}.h"]))
        for n, name in enumerate(EQT_TRANSFORMERS):
            tr, f = getattr(net, name), (fault if n == 0 else None)
            t[f"{name}.p"], t[f"{name}.att"] = _attention_emul(tr.attention, x, f)
            y1 = t[f"{name}.y1"] = _ln_emul(tr.norm1, x + t[f"{name}.att"], f)
            t[f"{name}.ff1"] = torch.relu(tr.ff.lin1(y1.permute(0, 2, 1))).permute(0, 2, 1).contiguous()
            t[f"{name}.ff2"] = tr.ff.lin2(t[f"{name}.ff1"].permute(0, 2, 1)).permute(0, 2, 1).contiguous()
            x = t[name] = tr.norm2(y1 + t[f"{name}.ff2"])
        t["decoder0.in"] = x
        for k, (lstm, att) in enumerate(zip(net.pick_lstms, net.pick_attentions)):
            f = fault if k == 0 else None
            h, c = _lstm_run(_lstm_w(lstm, ""), x, False, f if f in ("gnext", "step_rcp") else None)
            t[f"pick_lstms.{k}.h"], t[f"pick_lstms.{k}.c"] = h, c
            t[f"pick_attentions.{k}.p"], t[f"decoder{k + 1}.in"] = _attention_emul(att, h, f)
    return t
