"""GPU: the PhaseNet training step at the batch sizes where its launch shapes change form (csrc/train_phasenet.hip,
csrc/train_kernels.h, csrc/conv_train_b16.h).  The other training tests run even B at or near `max_batch`.  Each B-dependent
form, the batch sizes here that exercise it, and the assertion that catches a wrong result there:

- Weight gradients (wgrad_kernel, wgrad_bf16_kernel): WB = 2 windows per item for down3.down and up0.convT, 4 for
  down4.same, so groups = ceil(B / WB) ends in a partial group masked by `b0 + w < a.B` at B mod 4 = 1, 2, 3 (B = 2, 3, 37,
  65, 129, 511); from B = 129 on the grid hits wg_rows_cap (level 0 at 129, the deep layers at 511 and 1024) and one
  workgroup takes several items, whose rows sum_rows_multi_kernel folds.  Caught by check_every_kernel's "weight gradient" assertion, per layer.
- BatchNorm vector passes (bnv_*): GB = min(2048 / C, ceil(B / rows per block)) in [1, 256] over the strided window loop with
  `if (b >= a.B) continue`.  GB = 1 with a single partial row at B = 2 and 3; the deep layers step past GB = 1 at B = 129; level
  0 reaches the cap of 256 at B = 1024.  The bf16 conv launches leave the forward statistics as [cout][tiles x B][2].  Caught by
  check_every_kernel's ".a" (forward statistics), ".gz" and gamma / beta gradient assertions, and by
  check_adam_and_running_statistics's running mean / variance.
- Running variance: unbiased over N = B x L; N = 24 in the deepest layer at B = 2.  Caught by
  check_adam_and_running_statistics (ddof = 1).
- Bias gradient of `inc`: GB = B < 64 ? B : 64, below the switch at B = 2, 3, 37, above at 65, 129, 511, 1024.  Caught by
  check_every_kernel's "bias gradient" bound.
- Head: sum_rows_kernel<double, double> folds gx x B rows into 64 groups; at B = 2 in bf16 that is 6 rows and most groups
  are empty.  Caught by check_every_kernel's loss, prediction and out.weight / out.bias assertions.
- Buffers sized by max_batch that hold a larger step's windows past B - 1: every per-kernel case runs behind a max_batch
  step of other windows; test_reuse_after_a_larger_batch asks for bit identity with a fresh trainer.

No bar of tests/test_gpu_train_bf16.py is loosened here.  B = 1 is refused (tests/test_gpu_train.py::test_argument_errors).
"""
import hashlib

import numpy as np
import pytest
import torch

from oracle.models import load_pretrained
from tests.test_gpu_train import make_batch, torch_step
from tests.test_gpu_train_bf16 import _layers, check_adam_and_running_statistics, check_every_kernel
from volpick_amd import PhaseNet
from volpick_amd import generate as G
from volpick_amd.train import PhaseNetTrainer

pytestmark = pytest.mark.gpu

_FILL = {}


def filler(B):
    """Another batch of B windows: run first (update=False) so that every buffer holds a larger step's windows."""
    if B not in _FILL:
        _FILL[B] = make_batch(B, 4242 + B)
    return _FILL[B]


def one_step(B, dtype, max_batch, seed, fill=True):
    """One step (lr = 1e-3, Adam's first update) at B in a trainer built for max_batch, after a max_batch step that moved
    nothing but the running statistics (Adam's state stays untouched: update=False)."""
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=max_batch, dtype=dtype)
    if fill and max_batch > B:
        tr.step(*filler(max_batch), lr=1e-3, update=False)
    x, y = make_batch(B, seed)
    w0 = tr.weights()
    loss = tr.step(x, y, lr=1e-3, update=True)
    return dict(B=B, x=x, y=y, tr=tr, loss=loss, t=tr.tensors(B), g=tr.gradients(), pred=tr.predictions(B), w0=w0,
                w1=tr.weights(), mv=tr.adam_state())


def net_of(w0):
    """The oracle module carrying the weights the step's kernels read (the running statistics moved in the filler step)."""
    net = load_pretrained("phasenet")
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in w0.items()}, strict=False)
    return net


# ---- 1. odd and small batches, per kernel -----------------------------------------------------------------------------
# bf16 in a max_batch = 512 trainer (B = 511: one short of it); fp32 likewise.  B mod 4 = 1, 2, 3; 37 / 65 on both sides of
# the bias sum's switch at 64; 65 / 129 on both sides of the deep layers' BatchNorm step at 128; 2 the smallest legal batch.
SMALL = [("bf16", 2), ("bf16", 3), ("bf16", 37), ("bf16", 65), ("bf16", 129), ("bf16", 511),
         ("fp32", 3), ("fp32", 37), ("fp32", 129)]


@pytest.fixture(scope="module", params=SMALL, ids=[f"{d}-B{b}" for d, b in SMALL])
def small(request):
    dtype, B = request.param
    s = one_step(B, dtype, 512, 2024 + B)
    yield s
    s["tr"].close()


def test_every_kernel_at_odd_and_small_batches(small):
    s = small
    check_every_kernel(s["B"], s["x"], s["y"], s["tr"], s["loss"], s["t"], s["g"], s["pred"], net=net_of(s["w0"]))


def test_adam_and_running_statistics_at_odd_and_small_batches(small):
    s = small
    check_adam_and_running_statistics(s["g"], s["w0"], s["w1"], s["mv"], s["t"])


# ---- 2. B = 1024, the reference's other released batch size (configs_tune/p_1024_*.json) ------------------------------
@pytest.fixture(scope="module", params=["bf16", "fp32"])
def b1024(request):
    s = one_step(1024, request.param, 1024, 1024)
    s["dtype"] = request.param
    yield s
    s["tr"].close()


def _bn_output(z, bn):
    """u = BatchNorm(z) with the batch statistics of z itself (float64): the ReLU gate is u > 0."""
    z = z.astype(np.float64)
    mean, var = z.mean((0, 2)), z.var((0, 2))
    sc = bn.weight.detach().double().numpy() / np.sqrt(var + bn.eps)
    return z * sc[None, :, None] + (bn.bias.detach().double().numpy() - mean * sc)[None, :, None], sc


def fp32_end_to_end_against_autograd(s):
    """Tolerances of tests/test_gpu_train_large_batch.py::test_fp32_step_past_the_switch_matches_autograd (plain autograd, no
    storage rounding), with that test's ReLU-gate effect made explicit: an element of gz whose pre-activation sits within
    the z bar of zero takes the other side of the gate in one of the two, and its gradient is then the other gate's (seen at
    B = 1024: one element of up3.convT.gz at 0.32 of the tensor's maximum, the 99.9th percentile at 6.5e-7).  Such elements
    may exceed the 1e-1 bar -- at most 2e-6 of a tensor (at least one), as close_bf16's knife edges -- only when the kernel's
    gate (from its stored z) and torch's disagree there and torch's pre-activation lies within the z bar (5e-4 of max |z|,
    scaled by the channel's BatchNorm scale) of zero."""
    net = net_of(s["w0"])
    want_loss, grads, z, gz, pred = torch_step(net, s["x"], s["y"])
    assert abs(s["loss"] - want_loss) < 2e-6 * max(1.0, abs(want_loss)), (s["loss"], want_loss)
    assert np.abs(s["pred"] - pred).max() < 2e-5
    t = s["t"]
    bns = {name: bn for name, conv, bn, *_ in _layers(load_pretrained("phasenet"))}
    for name in z:
        e = float(np.abs(t[name + ".z"] - z[name]).max() / max(np.abs(z[name]).max(), 1e-30))
        assert e < 5e-4, (name + ".z", e)
        eg = np.abs(t[name + ".gz"] - gz[name]) / max(np.abs(gz[name]).max(), 1e-30)
        assert np.percentile(eg, 99.9) < 3e-3, (name + ".gz", float(np.percentile(eg, 99.9)))
        flipped = eg >= 1e-1
        if flipped.any():
            assert flipped.sum() <= max(1, int(2e-6 * flipped.size)), (name + ".gz", int(flipped.sum()), float(eg.max()))
            u_kernel, _ = _bn_output(t[name + ".z"], bns[name])
            u_torch, sc = _bn_output(z[name], bns[name])
            near = 5e-4 * np.abs(z[name]).max() * np.abs(sc)[None, :, None] * np.ones_like(u_torch)
            for b, c, j in np.argwhere(flipped):
                assert (u_kernel[b, c, j] > 0) != (u_torch[b, c, j] > 0), (name + ".gz", "beyond the bar, not a gate flip", (b, c, j))
                assert abs(u_torch[b, c, j]) <= near[b, c, j], (name + ".gz", "gate flip far from zero", (b, c, j), u_torch[b, c, j])


@pytest.mark.slow
def test_every_kernel_at_1024(b1024):
    """Every launch against torch on the inputs it read, with float64 references for the weight and BatchNorm-parameter
    gradients (B x 3001 = 3.1 M terms per sum at level 0); fp32 then also end to end against plain autograd (after the
    per-kernel check, so that a difference end to end is known to come from rounding carried through the chain)."""
    s = b1024
    check_every_kernel(s["B"], s["x"], s["y"], s["tr"], s["loss"], s["t"], s["g"], s["pred"], net=net_of(s["w0"]), ref64=True)
    if s["dtype"] == "fp32":
        fp32_end_to_end_against_autograd(s)


@pytest.mark.slow
def test_adam_and_running_statistics_at_1024(b1024):
    s = b1024
    check_adam_and_running_statistics(s["g"], s["w0"], s["w1"], s["mv"], s["t"])


# ---- 3. reuse after a larger batch ------------------------------------------------------------------------------------
def _digest(tr, B, loss):
    """Everything a step leaves, as digests of its bytes (bit identity without keeping the tensors)."""
    out = {"loss": np.float64(loss).tobytes().hex()}
    for k, v in tr.gradients().items():
        out["grad " + k] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    out["predictions"] = hashlib.sha256(tr.predictions(B).tobytes()).hexdigest()
    for k, v in tr.tensors(B).items():
        out[k] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    return out


def _fresh(B, max_batch, dtype, batch):
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=max_batch, dtype=dtype)
    try:
        return _digest(tr, B, tr.step(*batch, lr=1e-3, update=False))
    finally:
        tr.close()


def _same(got, want, what):
    diff = sorted(k for k in want if got[k] != want[k])
    assert got.keys() == want.keys() and not diff, (what, diff[:8], len(diff))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_reuse_after_a_larger_batch(dtype):
    """A max_batch = 512 trainer fed 512, 37, 3, 512 windows (update=False: the weights stay; the running statistics move but
    do not enter the training-mode forward): every step's loss, gradients, predictions and stored tensors equal, bit for bit,
    the first step of a fresh max_batch = 512 trainer at that B -- nothing of the larger step before it is read -- and the
    B = 37 step equals a fresh max_batch = 37 trainer's (no launch shape depends on max_batch)."""
    batches = {512: make_batch(512, 5120), 37: make_batch(37, 370), 3: make_batch(3, 30)}
    want = {B: _fresh(B, 512, dtype, batches[B]) for B in batches}
    _same(_fresh(37, 37, dtype, batches[37]), want[37], "B = 37: max_batch 37 against max_batch 512")
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=512, dtype=dtype)
    try:
        for k, B in enumerate([512, 37, 3, 512]):
            got = _digest(tr, B, tr.step(*batches[B], lr=1e-3, update=False))
            _same(got, want[B], f"step {k}: B = {B} behind larger steps")
    finally:
        tr.close()


# ---- 4. generated batches at odd B ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["window", "augmented"])
def test_step_bank_matches_step_at_odd_batches(kind, dtype, B):
    """step_bank (the batch generated in the trainer's own buffers) against step on make_batch's output of the same rows, in
    a max_batch = 64 trainer: loss, weights and the stored input bit for bit (as tests/test_gpu_augment.py at B = 64)."""
    from tests.test_gpu_generate import synthetic_bank

    w, ps, ss, bank = synthetic_bank(96, seed=3, device_tensor=True)
    try:
        a = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=64, dtype=dtype)
        b = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=64, dtype=dtype)
        if kind == "window":
            planner = G.WindowPlanner(bank, B, seed=5)
        else:
            planner = G.AugmentedPlanner(bank, B, np.arange(0, 64), np.arange(64, 96), seed=5, sigma=20,
                                         event_prob=(1, 1, 1), noise_prob=(1, 1, 1), gap_prob=(1, 1))
        epoch = planner.epoch()
        plans = [next(epoch) for _ in range(2)]
        assert all(len(rows) == B for rows in plans)
        for k, rows in enumerate(plans):
            batch = bank.make_batch(rows, a.model, 20)
            la = a.step_bank(bank, rows, lr=1e-3, sigma=20)
            lb = b.step(batch["X"], batch["y"], lr=1e-3)
            assert la == lb, (k, la, lb)
        wa, wb = a.weights(), b.weights()
        for key in wa:
            assert np.array_equal(wa[key], wb[key]), (key, float(np.abs(wa[key] - wb[key]).max()))
        xa, xb = a.tensors(B)["x"], b.tensors(B)["x"]
        assert np.array_equal(xa, xb)
        if dtype == "fp32":
            assert np.array_equal(xa, batch["X"].cpu().numpy())
        a.close()
        b.close()
    finally:
        bank.close()
