"""Float64 restatement of EQTransformer's pick branches in training -- ``pick_lstms.{0,1}`` (nn.LSTM(16, 16), 47 steps),
dropout, ``pick_attentions.{0,1}`` (oracle.models._SeqSelfAttention, band of 3) -- and of their backward pass, in plain numpy
and in pieces, so that every kernel of volpick_amd/csrc/train_eqt_pick.hip can be checked from the values it read.  Each
piece returns, beside its value, the sum of the absolute terms its rounding bar is counted from ("abs_..."): the same formula
with every product and sum taken over absolute values, (1 - tanh^2) and |tanh| bounded by 1.  Shared by
tests/test_eqt_pick_train_cpu.py (against float64 autograd of the oracle's own modules) and tests/test_gpu_eqt_pick_train.py.
Arrays are one branch's, laid out as the device lays them out: (B, rows, 47).

Bars.  On the CPU (restatement against float64 autograd): CPU_BAR = 512 * 2^-53 times the absolute terms -- a few hundred
float64 roundings, the two sides sum in different orders.  Two kinds of tensor have no abs_ terms that count the whole
computation, and take CHAIN = 64 times the bar instead, one factor for the depth of the 47-step recurrence behind them: the
forward tensors h, hd and v (terms 1, resp. 1 + |v|: values of magnitude <= 1), and the four LSTM weight gradients, whose
abs_ terms are those of the last sum alone (sum |gpre| |x|) while gpre itself comes through 47 steps of the adjoint.  The
one-step adjoint, ghd and the attention's weight gradients are held at the plain bar.

On the GPU (u = 2^-24; gamma_n = n u / (1 - n u) for a chain of n fp32 roundings, tests/eqt_dec_restate.py):

  pre-activation     gamma(34): b_ih + b_hh, 16 products with x_t, 16 with h_{t-1}, the joining sums
  sigmoid            5 u |p| + 2^-126, the bar of the decoder heads' sigmoid (expf to one ulp, a sum, a division)
  tanh               TANH_U = 6 u, absolute: tanhf is documented to 2 ulp, at most 4 u for |tanh| <= 1
  c                  gamma(3) (|f c'| + |i g|): a product and a fused multiply-add
  h                  |o| TANH_U + 2 u |h|
  hd                 exact: the fp32 product of h and the float scale 1 / (1 - drop_rate), or +0
  q, k               gamma(17): chains of 16 products
  scores e           sum_u |Wa_u| (7 u) + gamma(34) (sum_u |Wa_u tanh| + |ba|): the argument (q + k) + bh carries two roundings,
                     which move tanh by at most 2 u |x| (1 - tanh^2 x) < u; then 32 products and ba
  a                  a u (12 + 2 max_band |e - m|): e - m (u |e - m| into expf), expf (2 u), for numerator and denominator, the
                     band sum (2 u), + 1e-5 (u), the division (u)
  v                  gamma(3) sum |a hd|
  gv                 eqt_dec_restate.stage_backward of stage 0 at gamma(64 * 3 + 1), the decoder test's bar
  ghd, gq, gk        gamma(N_ATT = 160) abs: ga (16), the row's dot (3), ga - dot and the product with a (2), the maximum's share
                     (3) and its addition (1), 1 - tanh^2 of a recomputed tanh (16 u of its bound 1), the product G Wa (1 - s^2)
                     (2), gk's sum (3 + at most 47 argmax rows), the chain of 3 + 32 + 32 terms (67): 157
  gh                 exact from ghd, as hd is
  attention weights  gamma(100 + 188 B) abs: what precedes the last sum as above, then at most 4 * 47 terms per window (Wa; 47
                     for Wx, Wt, bh) over B windows
  gpre, gc           gamma(N_LSTM = 90) abs: gh + W_hh^T gpre_{t+1} (66), tanh c (6 u of 1) twice in 1 - tanh^2 (14 u), the
                     products and the fused multiply-add (8)
  LSTM weights       gamma(47 B + 2) sum |gpre| |x| (|h_{t-1}|; 1 for the biases)

What the per-kernel bars of the attention's adjoint can and cannot see: their abs_ terms take |ga| + |dot| where the kernel
forms ga - dot, a difference that nearly cancels on the released weights, so the bars stand two to three orders above the
device's rounding there and the maximum's share (2e-5 of the main term) is far below them.  They catch a wrong index, a
dropped term or a wrong sign of a main term; the argmax path is held by the end-to-end test against float64 autograd on the
weights with maxima outside the band, which tests/test_eqt_pick_train_cpu.py shows a backward without that path to miss.
The tie rule is held by the argmax the forward keeps and the backward reads: on weights whose score rows are all equal the
GPU test asserts it to be column 0, and the CPU test shows the restatement with that argmax to equal autograd.

The gradient of ba is exactly zero and is returned as 0.0.  Dropout: ``mask`` restates volpick_amd/csrc/philox.h."""
import numpy as np
import torch
import torch.nn as nn

from oracle import models as OM
from tests.augment_restate import philox4x32_10
from tests.eqt_dec_restate import FLOOR, U, gamma

T, H, G, NU, BAND, EPS = 47, 16, 64, 32, 3, float(OM.C.EQT_ATTENTION_EPS)
CPU_BAR = 512 * 2.0 ** -53
CHAIN = 64  # (the header: tensors behind the 47-step recurrence whose abs_ terms do not count it)
TANH_U = 6 * U
N_ATT, N_LSTM = 160, 90
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
ATT_KEYS = ("Wx", "Wt", "bh", "Wa", "ba")
N_FLOATS = 152261
DROP, SEED = 0.1, 20261021  # the dropout rate and seed of the GPU tests; the CPU tests check this seed's masks
SIX_SIGMA = 6 * np.sqrt(0.1 * 0.9 / (2 * 8 * 16 * 47))  # of the kept fraction of a B = 8 step's 12,032 elements: 0.0164


def is_pick_key(key):
    return key.startswith(("pick_lstms.", "pick_attentions."))


def branch_weights(state, k):
    """The nine tensors of branch k as float64 arrays by their short names."""
    w = {n: np.asarray(state[f"pick_lstms.{k}.{n}"], np.float64) for n in LSTM_KEYS}
    w.update({n: np.asarray(state[f"pick_attentions.{k}.{n}"], np.float64) for n in ATT_KEYS})
    return w


# ---- dropout ---------------------------------------------------------------------------------------------------------------------
def scale_of(drop_rate):
    """1 / (1 - drop_rate) as the library forms it: once, in float."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(drop_rate))


def mask(seed, step, B, drop_rate):
    """(2, B, 16, 47) float32 of 0 / 1: keep <=> (float)(w0 >> 8) 2^-24 >= drop_rate, w0 the first word of Philox4x32-10 at
    counter (b, (branch 16 + c) 47 + t, step low, step high) under key (seed low, seed high)."""
    k, b, c, t = np.meshgrid(np.arange(2), np.arange(B), np.arange(H), np.arange(T), indexing="ij")
    step = int(step)
    ctr = [b.ravel(), ((k * H + c) * T + t).ravel(), np.full(b.size, step & 0xFFFFFFFF), np.full(b.size, step >> 32)]
    w0 = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))[0]
    r = (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (r >= np.float32(drop_rate)).astype(np.float32).reshape(2, B, H, T)


def dropped(h, m, drop_rate):
    """hd in fp32 as the device forms it: h * scale where kept, +0 elsewhere (also the adjoint: gh from ghd)."""
    return np.where(m != 0, np.asarray(h, np.float32) * scale_of(drop_rate), np.float32(0.0)).astype(np.float32)


# ---- LSTM ------------------------------------------------------------------------------------------------------------------------
def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def _prev(a):
    """a_{t-1} along the last axis, zero at t = 0."""
    a = np.asarray(a, np.float64)
    return np.concatenate([np.zeros_like(a[..., :1]), a[..., :-1]], axis=-1)


def _next(a):
    a = np.asarray(a, np.float64)
    return np.concatenate([a[..., 1:], np.zeros_like(a[..., :1])], axis=-1)


def pre_activations(x, h, w):
    """(pre, abs) (B, 64, T) of every step from x (B, 16, T) and the h (B, 16, T) whose step t - 1 each step read."""
    x, hp = np.asarray(x, np.float64), _prev(h)
    b = w["bias_ih_l0"] + w["bias_hh_l0"]
    pre = np.einsum("rc,bct->brt", w["weight_ih_l0"], x) + np.einsum("ru,but->brt", w["weight_hh_l0"], hp) + b[None, :, None]
    ab = (np.einsum("rc,bct->brt", np.abs(w["weight_ih_l0"]), np.abs(x)) + np.einsum("ru,but->brt", np.abs(w["weight_hh_l0"]), np.abs(hp))
          + (np.abs(w["bias_ih_l0"]) + np.abs(w["bias_hh_l0"]))[None, :, None])
    return pre, ab


def gates(pre):
    """i, f, o = sigmoid, g = tanh of (B, 64, ...) rows in torch's order i, f, g, o."""
    pre = np.asarray(pre, np.float64)
    return np.concatenate([sigmoid(pre[:, :2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sigmoid(pre[:, 3 * H:])], axis=1)


def split(act):
    act = np.asarray(act, np.float64)
    return act[:, :H], act[:, H:2 * H], act[:, 2 * H:3 * H], act[:, 3 * H:]


def cell(act, c_prev):
    i, f, g, _ = split(act)
    c_prev = np.asarray(c_prev, np.float64)
    return f * c_prev + i * g, np.abs(f * c_prev) + np.abs(i * g)


def hidden(act, c):
    return split(act)[3] * np.tanh(np.asarray(c, np.float64))


def lstm_forward(x, w):
    """The recurrence step by step from zero state: dict pre, act, c, h, each (B, rows, T)."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    out = {k: np.zeros((B, n, T)) for k, n in (("pre", G), ("act", G), ("c", H), ("h", H))}
    h, c = np.zeros((B, H)), np.zeros((B, H))
    b = w["bias_ih_l0"] + w["bias_hh_l0"]
    for t in range(T):
        pre = x[:, :, t] @ w["weight_ih_l0"].T + h @ w["weight_hh_l0"].T + b
        act = gates(pre)
        c, _ = cell(act, c)
        h = hidden(act, c)
        for k, v in (("pre", pre), ("act", act), ("c", c), ("h", h)):
            out[k][:, :, t] = v
    return out


def lstm_step_backward(gh, gpre_next, gc, act, c, c_prev, w_hh):
    """One step of backpropagation through time from the values it reads: gh (the gradient arriving at h_t from outside),
    gpre_{t+1}, gc (the cell gradient entering the step, f_{t+1} dc_{t+1}), the step's gate activations, c_t, c_{t-1}.
    Arrays (B, rows, ...).  Returns dict gpre, gc_prev (= dc f, what step t - 1 receives) and their abs_ terms."""
    gh, gpre_next, gc, c, c_prev = (np.asarray(v, np.float64) for v in (gh, gpre_next, gc, c, c_prev))
    i, f, g, o = split(act)
    dh = gh + np.einsum("ru,br...->bu...", w_hh, gpre_next)
    abs_dh = np.abs(gh) + np.einsum("ru,br...->bu...", np.abs(w_hh), np.abs(gpre_next))
    tc = np.tanh(c)
    dc = gc + dh * o * (1.0 - tc * tc)
    abs_dc = np.abs(gc) + abs_dh * np.abs(o)
    gpre = np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
    abs_gpre = np.concatenate([abs_dc * np.abs(g * i * (1 - i)), abs_dc * np.abs(c_prev * f * (1 - f)), abs_dc * np.abs(i),
                               abs_dh * np.abs(o * (1 - o))], axis=1)
    return {"gpre": gpre, "gc_prev": dc * f, "abs_gpre": abs_gpre, "abs_gc_prev": abs_dc * np.abs(f)}


def lstm_backward_steps(gh, gpre, gc, act, c, w_hh):
    """Every step at once from the stored gpre_{t+1} and gc_t: (gpre, gc) as they should be, with abs_ terms.  gc[t] is what
    step t + 1 hands down, so the returned gc is the steps' gc_prev moved one step back, 0 at t = T - 1."""
    st = lstm_step_backward(gh, _next(gpre), gc, act, c, _prev(c), w_hh)
    return {"gpre": st["gpre"], "gc": _next(st["gc_prev"]), "abs_gpre": st["abs_gpre"], "abs_gc": _next(st["abs_gc_prev"])}


def lstm_backward(gh, act, c, w_hh):
    """The whole chain, t = T - 1 .. 0: gpre (B, 64, T) and the gc (B, 16, T) that entered each step."""
    B = np.asarray(gh).shape[0]
    gpre, gcs = np.zeros((B, G, T)), np.zeros((B, H, T))
    gc, nxt = np.zeros((B, H)), np.zeros((B, G))
    c = np.asarray(c, np.float64)
    for t in range(T - 1, -1, -1):
        gcs[:, :, t] = gc
        st = lstm_step_backward(gh[:, :, t], nxt, gc, act[:, :, t], c[:, :, t], c[:, :, t - 1] if t else np.zeros((B, H)), w_hh)
        gpre[:, :, t] = nxt = st["gpre"]
        gc = st["gc_prev"]
    return gpre, gcs


def lstm_weight_grads(gpre, x, h):
    """Sums over windows and steps: dict weight_ih_l0, weight_hh_l0, bias (both biases) with abs_ terms."""
    gpre, x, hp = np.asarray(gpre, np.float64), np.asarray(x, np.float64), _prev(h)
    return {"weight_ih_l0": np.einsum("brt,bct->rc", gpre, x), "abs_weight_ih_l0": np.einsum("brt,bct->rc", np.abs(gpre), np.abs(x)),
            "weight_hh_l0": np.einsum("brt,but->ru", gpre, hp), "abs_weight_hh_l0": np.einsum("brt,but->ru", np.abs(gpre), np.abs(hp)),
            "bias": gpre.sum((0, 2)), "abs_bias": np.abs(gpre).sum((0, 2))}


# ---- attention -------------------------------------------------------------------------------------------------------------------
def band():
    """(T, T) bool: column j of row i with i - 1 <= j < i + 2."""
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return (j >= i - BAND // 2) & (j < i - BAND // 2 + BAND)


def qk(hd, w):
    """q = hd Wt, k = hd Wx as (B, 32, T), with abs terms."""
    hd = np.asarray(hd, np.float64)
    f = lambda m, a: np.einsum("bct,cu->but", a, m)
    return f(w["Wt"], hd), f(w["Wx"], hd), f(np.abs(w["Wt"]), np.abs(hd)), f(np.abs(w["Wx"]), np.abs(hd))


def _tanh_terms(q, k, w):
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    return np.tanh(q.transpose(0, 2, 1)[:, :, None, :] + k.transpose(0, 2, 1)[:, None, :, :] + w["bh"])  # (B, i, j, u)


def scores(q, k, w):
    """e (B, T, T) and its bar's terms: (e, sum_u |Wa_u|, sum_u |Wa_u tanh| + |ba|)."""
    s = _tanh_terms(q, k, w)
    wa = w["Wa"][:, 0]
    return s @ wa + w["ba"][0], float(np.abs(wa).sum()), np.abs(s) @ np.abs(wa) + abs(w["ba"][0])


def weights_of(e):
    """(a, argmax, max over the band of |e - m|) from the scores: exp(e - full-row max), band, / (sum + 1e-5); argmax is the
    lowest index among equal maxima (torch.max(dim))."""
    e = np.asarray(e, np.float64)
    arg = np.argmax(e, axis=-1)
    d = e - e.max(-1, keepdims=True)
    p = np.where(band(), np.exp(d), 0.0)
    return p / (p.sum(-1, keepdims=True) + EPS), arg, np.where(band(), np.abs(d), 0.0).max(-1, keepdims=True)


def context(a, hd):
    """v (B, 16, T) = sum_j a_ij hd_j, with abs terms."""
    a, hd = np.asarray(a, np.float64), np.asarray(hd, np.float64)
    return np.einsum("bij,bcj->bci", a, hd), np.einsum("bij,bcj->bci", np.abs(a), np.abs(hd))


def attention_forward(hd, w):
    q, k, _, _ = qk(hd, w)
    e, _, _ = scores(q, k, w)
    a, arg, _ = weights_of(e)
    return {"q": q, "k": k, "e": e, "a": a, "argmax": arg, "v": context(a, hd)[0]}


def attention_backward(gv, hd, q, k, a, argmax, w, argmax_path=True):
    """The adjoint from the values the kernel reads: gv (B, 16, T), hd, q, k, a and the kept argmax (B, T).  Returns dict ghd,
    gq, gk (device layouts) and the sums over windows Wx, Wt, bh, Wa, ba (= 0.0), each with its abs_ terms.
    ``argmax_path=False`` plants the fault of a backward that treats the row maximum as a constant."""
    gv, hd, a = (np.asarray(v, np.float64) for v in (gv, hd, a))
    B = gv.shape[0]
    argmax = np.asarray(argmax).astype(np.int64).reshape(B, T)
    inb = band()
    s = _tanh_terms(q, k, w)
    wa = w["Wa"][:, 0]
    out = {}
    for tag, f in (("", lambda v: v), ("abs_", np.abs)):
        ab = tag == "abs_"
        ga = np.einsum("bci,bcj->bij", f(gv), f(hd)) * inb  # dL/da in the band
        dot = (f(a) * ga).sum(-1, keepdims=True)
        ge = f(a) * ((ga + dot) if ab else (ga - dot))  # dL/de of the band's columns through p = exp(e - m)
        gm = ge.sum(-1) if ab else -ge.sum(-1)  # ... and through m: 1e-5 is not shifted with the row
        if argmax_path:
            ge = ge.copy()
            np.add.at(ge, (np.arange(B)[:, None], np.arange(T)[None, :], argmax), gm)
        used = inb[None] | (ge != 0)
        d = ge[..., None] * f(wa) * (np.ones_like(s) if ab else (1.0 - s * s)) * used[..., None]  # d / d tanh argument (B, i, j, u)
        gq, gk = d.sum(2).transpose(0, 2, 1), d.sum(1).transpose(0, 2, 1)  # (B, u, T)
        out[tag + "gq"], out[tag + "gk"] = gq, gk
        out[tag + "ghd"] = (np.einsum("bij,bci->bcj", f(a), f(gv)) + np.einsum("cu,but->bct", f(w["Wt"]), gq)
                            + np.einsum("cu,but->bct", f(w["Wx"]), gk))
        out[tag + "Wt"] = np.einsum("bct,but->cu", f(hd), gq)
        out[tag + "Wx"] = np.einsum("bct,but->cu", f(hd), gk)
        out[tag + "bh"] = d.sum((0, 1, 2))
        out[tag + "Wa"] = (ge[..., None] * (np.ones_like(s) if ab else s) * used[..., None]).sum((0, 1, 2))[:, None]
    out["ba"], out["abs_ba"] = np.zeros(1), np.zeros(1)
    return out


# ---- the oracle's own modules ----------------------------------------------------------------------------------------------------
class PickBranch(nn.Module):
    """nn.LSTM(16, 16) -> (dropout mask and scale, given) -> _SeqSelfAttention(16, band 3), by the oracle's classes."""

    def __init__(self):
        super().__init__()
        self.lstm = nn.LSTM(16, 16)
        self.att = OM._SeqSelfAttention(16, attention_width=OM.C.PICK_ATTENTION_WIDTH)

    def forward(self, x, m=None, scale=1.0):
        """x (B, 16, T) -> (h, hd, v), each (B, 16, T)."""
        h = self.lstm(x.permute(2, 0, 1))[0].permute(1, 2, 0)
        hd = h if m is None else h * m * scale
        return h, hd, self.att(hd)[0]


def build_branch(state, k, dtype=torch.float64):
    net = PickBranch()
    sd = {f"lstm.{n}": torch.as_tensor(np.asarray(state[f"pick_lstms.{k}.{n}"])) for n in LSTM_KEYS}
    sd.update({f"att.{n}": torch.as_tensor(np.asarray(state[f"pick_attentions.{k}.{n}"])) for n in ATT_KEYS})
    net.load_state_dict(sd, strict=True)
    return net.to(dtype)


def branch_autograd(state, k, x, gv, m=None, scale=1.0, dtype=torch.float64):
    """Autograd of sum(v * gv) through branch k: dict of h, hd, v, their gradients gh, ghd, and the nine weight gradients by
    short name."""
    net = build_branch(state, k, dtype)
    xt = torch.as_tensor(np.asarray(x)).to(dtype)
    mt = None if m is None else torch.as_tensor(np.asarray(m)).to(dtype)
    h, hd, v = net(xt, mt, float(scale))
    h.retain_grad()
    if hd is not h:
        hd.retain_grad()
    (v * torch.as_tensor(np.asarray(gv)).to(dtype)).sum().backward()
    out = {"h": h, "hd": hd, "v": v, "gh": h.grad, "ghd": hd.grad}
    out.update({n.split(".", 1)[1]: p.grad for n, p in net.named_parameters()})
    return {n: t.detach().numpy().astype(np.float64) for n, t in out.items()}


def restated_gradients(state, k, x, gv, m=None, drop_rate=0.0, argmax_path=True):
    """The same through the restatement in float64: forward from x, backward from gv; dict with the nine weight gradients (and
    abs_ terms of the attention's) and the intermediate tensors."""
    w = branch_weights(state, k)
    fw = lstm_forward(x, w)
    sc = float(scale_of(drop_rate)) if m is not None else 1.0
    keep = np.ones_like(fw["h"]) if m is None else np.asarray(m, np.float64)
    hd = fw["h"] * keep * sc
    att = attention_forward(hd, w)
    bk = attention_backward(gv, hd, att["q"], att["k"], att["a"], att["argmax"], w, argmax_path)
    gh = bk["ghd"] * keep * sc
    gpre, gc = lstm_backward(gh, fw["act"], fw["c"], w["weight_hh_l0"])
    lw = lstm_weight_grads(gpre, x, fw["h"])
    out = dict(fw, hd=hd, gh=gh, gpre=gpre, gc=gc, **att)
    out.update({n: bk[n] for n in bk})
    out.update({"weight_ih_l0": lw["weight_ih_l0"], "weight_hh_l0": lw["weight_hh_l0"], "bias_ih_l0": lw["bias"], "bias_hh_l0": lw["bias"],
                "abs_weight_ih_l0": lw["abs_weight_ih_l0"], "abs_weight_hh_l0": lw["abs_weight_hh_l0"], "abs_bias_ih_l0": lw["abs_bias"],
                "abs_bias_hh_l0": lw["abs_bias"]})
    return out
