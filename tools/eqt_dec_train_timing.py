"""What one training step of EQTransformer's decoder stacks costs (``EQTransformerDecoderTrainer``, ``vp_eqt_dec_train_step``)
at B = 256 on a device-resident batch, beside stock PyTorch-ROCm doing the same work on the same GPU in the same run.

Ours: HIP events inside the library between the step's phases (``set_timing``): trunk (the frozen inference launches up to
``decoder.in``), forward (seven stages, heads, float64 loss), input gradients, weight gradients, Adam; the step is their
sum.  PyTorch: eager fp32, ``torch.optim.Adam``, forward + backward + update of the same three decoders and heads from the
same ``decoder.in`` and labels (it runs no trunk), ``torch.cuda.Event`` around each step.  After --warmup steps of each, the
two take turns in blocks of ten steps until each has run --steps; median [min .. max] per step.  The floor is arithmetic,
not a measurement: the decoders' forward MACs, three times (forward, input gradient, weight gradient), at the fp32 matrix
peak.

    python tools/eqt_dec_train_timing.py [--batch 256] [--steps 50] [--warmup 10] [--out FILE]

``--scope pick_branches``: the step of ``EQTransformerDecoderTrainer(scope="pick_branches")`` (dropout 0.1) beside the
scope-0 step of a second trainer in the same run, the three pick parts alone (``pick_ms``: forward, adjoints, weight
gradients; events inside the library), and stock PyTorch-ROCm (eager, fp32) doing forward and backward of the same two
``nn.LSTM(16, 16)`` + ``nn.Dropout(0.1)`` + attention branches from the same ``pick.x``, with the decoders' ``pick.gv`` as the
incoming gradient.  The three take turns in blocks of ten steps.  Writes profiles/eqt_pick_train_timing.txt.
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import models as OM  # noqa: E402
from volpick_amd import EQTransformer, _lib  # noqa: E402
from volpick_amd.synthetic import synthetic_windows  # noqa: E402
from volpick_amd.train import EQT_LOSS_WEIGHTS, EQTransformerDecoderTrainer  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12  # FLOP/s, the data sheet
T = 6000
DOUT, DCI, DCO, DK = (94, 188, 375, 750, 1500, 3000, 6000), (16, 64, 64, 32, 32, 16, 16), (64, 64, 32, 32, 16, 16, 8), (3, 5, 5, 7, 7, 9, 11)
PHASES = ("trunk", "forward + heads + loss", "input gradients", "weight gradients", "Adam")


class DecoderHeads(nn.Module):
    """The three decoders and heads of the oracle's EQTransformer, by its names."""

    def __init__(self):
        super().__init__()
        f, k = list(OM.C.EQT_FILTERS), list(OM.C.EQT_KERNELS)
        self.decoder_d = OM._Decoder(16, f[::-1], k[::-1], T)
        self.conv_d = nn.Conv1d(f[0], 1, 11, padding=5)
        self.pick_decoders = nn.ModuleList(OM._Decoder(16, f[::-1], k[::-1], T) for _ in range(2))
        self.pick_convs = nn.ModuleList(nn.Conv1d(f[0], 1, 11, padding=5) for _ in range(2))

    def forward(self, dec_in):
        decs = [self.decoder_d, self.pick_decoders[0], self.pick_decoders[1]]
        heads = [self.conv_d, self.pick_convs[0], self.pick_convs[1]]
        return [torch.sigmoid(h(d(dec_in[i]))).squeeze(1) for i, (d, h) in enumerate(zip(decs, heads))]


def batch(B, seed=1):
    rng = np.random.default_rng(seed)
    x = synthetic_windows(B, T, seed=seed).astype(np.float64)
    x -= x.mean(-1, keepdims=True)
    x /= np.abs(x).max((1, 2), keepdims=True)
    t = np.arange(T)
    y = np.zeros((B, 3, T), np.float32)
    for b in range(B):
        p = rng.uniform(300, 3000)
        s = p + rng.uniform(200, 1200)
        y[b, 1] = np.exp(-((t - p) ** 2) / 800.0)
        y[b, 2] = np.exp(-((t - s) ** 2) / 800.0)
        y[b, 0, int(p):int(s + 1.4 * (s - p))] = 1.0
    return torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(y).cuda()


def spread(v):
    return f"{statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}]"


class BandAttention(OM._SeqSelfAttention):
    """The oracle's attention, its forward restated with the band mask built on the input's device."""

    def forward(self, x):
        x = x.permute(0, 2, 1)
        q = torch.matmul(x, self.Wt).unsqueeze(2)
        k = torch.matmul(x, self.Wx).unsqueeze(1)
        e = (torch.matmul(torch.tanh(q + k + self.bh), self.Wa) + self.ba).squeeze(-1)
        e = torch.exp(e - e.max(dim=-1, keepdim=True).values)
        t = torch.arange(e.shape[1], device=e.device)
        lower = t - self.attention_width // 2
        mask = torch.logical_and(lower <= t.unsqueeze(1), t.unsqueeze(1) < lower + self.attention_width)
        e = torch.where(mask, e, torch.zeros_like(e))
        a = e / (e.sum(dim=-1, keepdim=True) + self.eps)
        return torch.matmul(a, x).permute(0, 2, 1), a


class PickBranches(nn.Module):
    """pick_lstms / pick_attentions of the oracle's EQTransformer with SeisBench's dropout between them."""

    def __init__(self, drop_rate):
        super().__init__()
        self.pick_lstms = nn.ModuleList(nn.LSTM(16, 16) for _ in range(2))
        self.pick_attentions = nn.ModuleList(BandAttention(16, attention_width=OM.C.PICK_ATTENTION_WIDTH) for _ in range(2))
        self.drop = nn.Dropout(drop_rate)

    def forward(self, x):
        out = []
        for lstm, att in zip(self.pick_lstms, self.pick_attentions):
            px = self.drop(lstm(x.permute(2, 0, 1))[0].permute(1, 2, 0))
            out.append(att(px)[0])
        return torch.stack(out)


def read_tensor(tr, wanted, B):
    """One tensor of the last step by name (``tensors()`` would copy every tensor of the step, gigabytes at B = 256)."""
    lib = tr._lib
    for i in range(lib.vp_eqt_dec_train_tensor_count(tr._h)):
        name, s, c, l = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(lib.vp_eqt_dec_train_tensor_info(tr._h, i, C.byref(name), C.byref(s), C.byref(c), C.byref(l)))
        if name.value.decode() == wanted:
            out = np.empty((s.value, B, c.value, l.value), dtype=np.float32)
            _lib.check(lib.vp_eqt_dec_train_tensor_read(tr._h, i, B, _lib.ptr(out)))
            return out[0] if s.value == 1 else out
    raise KeyError(wanted)


def main_pick(a):
    B = a.batch
    x, y = batch(B)
    make = lambda scope: EQTransformerDecoderTrainer(EQTransformer.from_pretrained("volpick"), max_batch=B, scope=scope)
    pick, dec = make("pick_branches"), make("decoders")
    for tr in (pick, dec):
        tr.set_timing(True)
        tr.step(x, y, 0.0, EQT_LOSS_WEIGHTS, update=False)
    px, gv = (torch.from_numpy(read_tensor(pick, name, B)).cuda() for name in ("pick.x", "pick.gv"))
    net = PickBranches(pick.drop_rate)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in pick.weights().items() if k.startswith(("pick_lstms", "pick_att"))})
    net = net.cuda().train()

    def torch_step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        net.zero_grad(set_to_none=True)
        net(px).backward(gv)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def pick_step():
        pick.step(x, y, 1e-3, EQT_LOSS_WEIGHTS)
        return sum(pick.phase_ms()), pick.pick_ms()

    def dec_step():
        dec.step(x, y, 1e-3, EQT_LOSS_WEIGHTS)
        return sum(dec.phase_ms())

    for _ in range(a.warmup):
        pick_step(), dec_step(), torch_step()
    whole, parts, base, theirs = [], [], [], []
    while len(whole) < a.steps:
        n = min(10, a.steps - len(whole))
        for _ in range(n):
            ms, p = pick_step()
            whole.append(ms), parts.append(p)
        base += [dec_step() for _ in range(n)]
        theirs += [torch_step() for _ in range(n)]
    psum = [sum(p) for p in parts]
    med = statistics.median
    added = med(whole) - med(base)
    iqr = lambda v: statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0]
    lines = [f"EQTransformer training step with the pick branches, B = {B}, fp32, dropout {pick.drop_rate}, {torch.cuda.get_device_name(0)}",
             f"{a.steps} steps each after {a.warmup} warm-up steps, in turns of ten; ms per step, median [min .. max]", "",
             f"scope pick_branches, whole step             {spread(whole)}   {pick.launch_count()} launches",
             f"scope decoders, whole step                  {spread(base)}   {dec.launch_count()} launches"]
    lines += [f"    pick {name:<35}{spread([p[i] for p in parts])}" for i, name in enumerate(("forward", "adjoints", "weight gradients"))]
    lines += [f"    pick parts together                     {spread(psum)}",
              f"PyTorch eager, the two branches fwd + bwd   {spread(theirs)}", "",
              f"pick parts together / PyTorch               {med(psum) / med(theirs):.3f}",
              f"added to the scope-0 step (difference of the medians) {added:.3f} ms; the parts' sum {med(psum):.3f} ms",
              f"step-to-step spread (interquartile range): scope pick_branches {iqr(whole):.3f} ms, scope decoders {iqr(base):.3f} ms"]
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    pick.close(), dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scope", choices=("decoders", "pick_branches"), default="decoders")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.out is None:
        a.out = str(ROOT / "profiles" / ("eqt_dec_train_timing.txt" if a.scope == "decoders" else "eqt_pick_train_timing.txt"))
    if a.scope == "pick_branches":
        return main_pick(a)
    B = a.batch
    model = EQTransformer.from_pretrained("volpick")
    tr = EQTransformerDecoderTrainer(model, max_batch=B)
    tr.set_timing(True)
    x, y = batch(B)
    tr.step(x, y, 0.0, EQT_LOSS_WEIGHTS, update=False)
    dec_in = torch.from_numpy(tr.tensors(B)["decoder.in"]).cuda()

    net = DecoderHeads()
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in tr.weights().items()}, strict=True)
    net = net.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    bce = nn.BCELoss()

    def torch_step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opt.zero_grad(set_to_none=True)
        p = net(dec_in)
        loss = sum(w * bce(p[h], y[:, h]) for h, w in enumerate(EQT_LOSS_WEIGHTS))
        loss.backward()
        opt.step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), float(loss.detach())

    def our_step():
        loss = tr.step(x, y, 1e-3, EQT_LOSS_WEIGHTS)
        return tr.phase_ms(), loss

    for _ in range(a.warmup):
        our_step(), torch_step()
    ours, theirs, our_loss, their_loss = [], [], [], []
    while len(ours) < a.steps:
        for _ in range(min(10, a.steps - len(ours))):
            ms, loss = our_step()
            ours.append(ms), our_loss.append(loss)
        for _ in range(min(10, a.steps - len(theirs))):
            ms, loss = torch_step()
            theirs.append(ms), their_loss.append(loss)
    total = [sum(ms) for ms in ours]
    decoders = [sum(ms[1:]) for ms in ours]
    flop = 3 * 3 * sum(2.0 * co * ci * k * lo for co, ci, k, lo in zip(DCO, DCI, DK, DOUT)) * B
    floor_ms = flop / FP32_MATRIX_PEAK * 1e3
    med, med_dec, med_t = statistics.median(total), statistics.median(decoders), statistics.median(theirs)
    lines = [f"EQTransformer decoder training step, B = {B}, fp32, {torch.cuda.get_device_name(0)}",
             f"{a.steps} steps each after {a.warmup} warm-up steps, in turns of ten; ms per step, median [min .. max]", "",
             f"this library, whole step (trunk included)   {spread(total)}   {tr.launch_count()} launches"]
    lines += [f"    {name:<40}{spread([ms[i] for ms in ours])}" for i, name in enumerate(PHASES)]
    lines += [f"this library, decoders alone (no trunk)     {spread(decoders)}",
              f"PyTorch eager + torch.optim.Adam (no trunk) {spread(theirs)}", "",
              f"decoders alone / PyTorch                    {med_dec / med_t:.3f}",
              f"whole step / PyTorch                        {med / med_t:.3f}",
              f"arithmetic floor: {flop / 1e9:.1f} GFLOP at {FP32_MATRIX_PEAK / 1e12:.1f} TFLOP/s = {floor_ms:.3f} ms; "
              f"decoders alone / floor = {med_dec / floor_ms:.2f}",
              f"loss of the first / last timed step: this library {our_loss[0]:.6g} / {our_loss[-1]:.6g}, PyTorch "
              f"{their_loss[0]:.6g} / {their_loss[-1]:.6g}"]
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    tr.close()


if __name__ == "__main__":
    main()
