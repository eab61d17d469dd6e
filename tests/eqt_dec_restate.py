"""Float64 restatement of what ``EQTransformerDecoderTrainer`` trains: the three decoder stacks and heads of EQTransformer,
fed ``decoder.in``, with the loss of ``EQTransformerLit.shared_step`` -- built from ``oracle.models._Decoder`` and torch
autograd on the CPU -- and plain-numpy formulas of ONE stage's forward and backward pass for the per-kernel checks, each with
the sum of the absolute terms its rounding bar is counted from.  Shared by tests/test_eqt_dec_train_cpu.py and
tests/test_gpu_eqt_dec_train.py.

Rounding bars (u = 2^-24): an fp32 FMA chain of n terms in any order errs by at most gamma_n sum|terms|,
gamma_n = n u / (1 - n u).  n per kernel, as volpick_amd/csrc/train_eqt_dec.hip forms it:

  stage forward      Cin K + 1     the accumulator starts at the bias, then Cin K products
  input gradient     Cout K + 1    the chain of gu[2j] (gu[2j+1]) and the pair sum of the up-sample's adjoint
  weight gradient    B T_out       every product gz u of the element, whatever workgroup summed it first
  bias gradient      B T_out
  head logit         8 * 11 + 1
  head input grad.   11
  sigmoid            p = 1 / (1 + expf(-z)): expf to one ulp (2 u), the sum (u, weighted e / (1 + e) < 1) and the division
                     (u): 4 u, taken as 5 u |p|, plus 2^-126 for a denormal p.
  dLoss/dlogit       ((p - y) / max((1 - p) p, 1e-12) * w) / (B T) * (1 - p) * p, ten roundings of factors of one product
                     ((p - y), (1 - p) used twice, the product q, the division, * w, / (B T), * (1 - p), * p, the float of
                     B T): 12 u |g| + 2^-126.
"""
import numpy as np
import torch
import torch.nn as nn

from oracle import models as OM

U = 2.0 ** -24
FLOOR = 2.0 ** -126
DIN = (47, 94, 188, 375, 750, 1500, 3000)
DOUT = (94, 188, 375, 750, 1500, 3000, 6000)
DCI = (16, 64, 64, 32, 32, 16, 16)
DCO = (64, 64, 32, 32, 16, 16, 8)
DK = (3, 5, 5, 7, 7, 9, 11)
DEC_PREFIX = ("decoder_d", "pick_decoders.0", "pick_decoders.1")
HEAD_PREFIX = ("conv_d", "pick_convs.0", "pick_convs.1")
N_FLOATS = 145731


def gamma(n):
    return n * U / (1.0 - n * U)


def is_decoder_key(key):
    return any(key.startswith(p + ".") for p in DEC_PREFIX + HEAD_PREFIX)


class DecoderHeads(nn.Module):
    """decoder_d / conv_d and pick_decoders / pick_convs of ``oracle.models.EQTransformer``, by the same names."""

    def __init__(self):
        super().__init__()
        f, k = list(OM.C.EQT_FILTERS), list(OM.C.EQT_KERNELS)
        self.decoder_d = OM._Decoder(16, f[::-1], k[::-1], 6000)
        self.conv_d = nn.Conv1d(f[0], 1, 11, padding=5)
        self.pick_decoders = nn.ModuleList(OM._Decoder(16, f[::-1], k[::-1], 6000) for _ in range(2))
        self.pick_convs = nn.ModuleList(nn.Conv1d(f[0], 1, 11, padding=5) for _ in range(2))

    def forward(self, dec_in):
        """dec_in (3, B, 16, 47) -> predictions (B, 3, 6000): detection, P, S."""
        decs = [self.decoder_d, self.pick_decoders[0], self.pick_decoders[1]]
        heads = [self.conv_d, self.pick_convs[0], self.pick_convs[1]]
        return torch.stack([torch.sigmoid(h(d(dec_in[i]))).squeeze(1) for i, (d, h) in enumerate(zip(decs, heads))], dim=1)


def build(state, dtype=torch.float64):
    """The module with the 48 tensors of ``state`` (name -> array; other keys are ignored)."""
    net = DecoderHeads()
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state.items() if is_decoder_key(k)}, strict=True)
    return net.to(dtype)


def loss_of(net, dec_in, y, weights):
    """``sum_h weights[h] BCELoss(p[:, h], y[:, h])`` (mean reduction per head) as a tensor."""
    p = net(dec_in)
    bce = nn.BCELoss()
    return sum(float(w) * bce(p[:, h], y[:, h]) for h, w in enumerate(weights))


def loss_and_grads(state, dec_in, y, weights, dtype=torch.float64):
    """(loss, {name: gradient}) of the restatement in ``dtype`` by autograd."""
    net = build(state, dtype)
    loss = loss_of(net, torch.as_tensor(np.asarray(dec_in)).to(dtype), torch.as_tensor(np.asarray(y)).to(dtype), weights)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy().astype(np.float64) for k, p in net.named_parameters()}


def adam_train(state, dec_in, y, weights, lr, steps, dtype=torch.float64):
    """Losses of ``steps`` Adam steps (torch's defaults) on one fixed batch, and the final state."""
    net = build(state, dtype)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    x, t = torch.as_tensor(np.asarray(dec_in)).to(dtype), torch.as_tensor(np.asarray(y)).to(dtype)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_of(net, x, t, weights)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach().numpy() for k, v in net.state_dict().items()}


# ---- one stage in plain numpy (float64) ------------------------------------------------------------------------------------
def upsampled(x, lout):
    """Nearest x2 up-sample of (..., C, L) cropped to ``lout`` (2 L or 2 L - 1)."""
    return np.repeat(np.asarray(x, np.float64), 2, axis=-1)[..., :lout]


def _conv(u, w, drop_tap=None):
    """sum_ci sum_k w[co][ci][k] u[..., ci, t + k - pad], zero padding: (..., Cout, L)."""
    K, pad, L = w.shape[2], w.shape[2] // 2, u.shape[-1]
    up = np.pad(u, [(0, 0)] * (u.ndim - 1) + [(pad, pad)])
    out = np.zeros(u.shape[:-2] + (w.shape[0], L))
    for k in range(K):
        if k != drop_tap:
            out += np.einsum("oc,...ct->...ot", w[:, :, k], up[..., k:k + L])
    return out


def stage_forward(x, w, b, lout):
    """(a, sum of the absolute terms): a = relu(conv(up(x)) + b)."""
    w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
    u = upsampled(x, lout)
    z = _conv(u, w) + b[:, None]
    return np.maximum(z, 0.0), _conv(np.abs(u), np.abs(w)) + np.abs(b)[:, None]


def stage_backward(x, a, ga, w, lout, fault=None):
    """The backward pass of one stage from its input x (B, Cin, Lin), its output a and the gradient ga with respect to a
    (B, Cout, lout).  Returns a dict: gz, ga_in (B, Cin, Lin), gw, gb and the sums of the absolute terms abs_ga_in, abs_gw,
    abs_gb.  ``fault`` plants one of the mistakes the tests must see: "crop" (gu[lout] added into the last ga of a cropped
    stage), "mask_ge" (ReLU mask a >= 0), "drop_tap" (the last tap left out), "bias_one_window"."""
    x, a, ga, w = (np.asarray(v, np.float64) for v in (x, a, ga, w))
    K, pad, lin = w.shape[2], w.shape[2] // 2, x.shape[-1]
    gz = ga * ((a >= 0) if fault == "mask_ge" else (a > 0))
    u = upsampled(x, lout)
    drop = K - 1 if fault == "drop_tap" else None
    # gu[ci][s] = sum_co sum_k gz[co][s - k + pad] w[co][ci][k], s in [0, 2 lin): the conv of gz with the flipped, transposed taps
    wt = np.ascontiguousarray(w.transpose(1, 0, 2)[:, :, ::-1])
    ext = np.pad(gz, [(0, 0), (0, 0), (0, 2 * lin - lout)])  # the row as if it went on: gz is zero behind lout
    gu = _conv(ext, wt, None if drop is None else K - 1 - drop)
    abs_gu = _conv(np.abs(ext), np.abs(wt))
    if fault != "crop":
        gu[..., lout:] = 0.0
    abs_gu[..., lout:] = 0.0
    ga_in = gu[..., 0::2] + gu[..., 1::2]
    up = np.pad(u, [(0, 0), (0, 0), (pad, pad)])
    gw, abs_gw = np.zeros(w.shape), np.zeros(w.shape)
    for k in range(K):
        if k != drop:
            gw[:, :, k] = np.einsum("bot,bct->oc", gz, up[..., k:k + lout])
        abs_gw[:, :, k] = np.einsum("bot,bct->oc", np.abs(gz), np.abs(up[..., k:k + lout]))
    gb = (gz[:1] if fault == "bias_one_window" else gz).sum((0, 2))
    return {"gz": gz, "ga_in": ga_in, "gw": gw, "gb": gb, "abs_ga_in": abs_gu[..., 0::2] + abs_gu[..., 1::2], "abs_gw": abs_gw,
            "abs_gb": np.abs(gz).sum((0, 2))}


def head_forward(a6, w, b):
    """(z, sum of the absolute terms) of Conv1d(8, 1, 11, padding 5): a6 (B, 8, T) -> (B, T)."""
    w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
    a6 = np.asarray(a6, np.float64)
    return _conv(a6, w)[:, 0] + b[0], _conv(np.abs(a6), np.abs(w))[:, 0] + abs(b[0])


def sigmoid(z):
    z = np.asarray(z, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def head_gradient(p, y, weight, numel):
    """dLoss/dlogit of one head from fp32 p and y as torch forms it; ``weight`` and ``numel`` as the kernel holds them (fp32)."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    q = (1.0 - p) * p
    return (p - y) / np.maximum(q, 1e-12) * float(np.float32(weight)) / float(np.float32(numel)) * (1.0 - p) * p


def head_backward(gz, a6, w):
    """ga6 (B, 8, T), gw (1, 8, 11), gb (1,) of the head conv from gz (B, T), with the sums of the absolute terms."""
    gz, a6, w = np.asarray(gz, np.float64)[:, None], np.asarray(a6, np.float64), np.asarray(w, np.float64)
    wt = np.ascontiguousarray(w.transpose(1, 0, 2)[:, :, ::-1])
    T = a6.shape[-1]
    ap = np.pad(a6, [(0, 0), (0, 0), (5, 5)])
    gw = np.stack([np.einsum("bot,bct->oc", gz, ap[..., k:k + T]) for k in range(11)], axis=-1)
    abs_gw = np.stack([np.einsum("bot,bct->oc", np.abs(gz), np.abs(ap[..., k:k + T])) for k in range(11)], axis=-1)
    return {"ga6": _conv(gz, wt), "abs_ga6": _conv(np.abs(gz), np.abs(wt)), "gw": gw, "abs_gw": abs_gw, "gb": gz.sum((0, 2)),
            "abs_gb": np.abs(gz).sum((0, 2))}


def edge_samples(lout, k):
    """The output samples of a stage the checks name explicitly: the first and last k // 2, and t = 373, 374 at the crop."""
    h = max(k // 2, 1)
    s = set(range(h)) | set(range(lout - h, lout))
    if lout == 375:
        s |= {373, 374}
    return sorted(s)
