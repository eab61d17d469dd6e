"""GPU parity of the bf16 training step AT THE BATCH THE BENCH TIMES (BASELINE configs[4]; contract:
the reference's volpick/model/models.py:34-51,160-164 and model_training/configs_tune/p_512_5e-04_ga20_400_s.json: batch 512).

Round 4 verified the step at B = 6 / 8 / 40 and timed it at B = 512; the trainer changes form with the batch
(`csrc/train_phasenet.hip`: the grid-stride BatchNorm passes `a.GB`, `GB = B < 64 ? B : 64` of the bias sum, the capped
weight-gradient grids with several work items per workgroup, the two-stream weight-gradient overlap).  Here one step at
B = 128 (first size past the switch) and one at B = 512 go through the same layer-by-layer check as B = 6: every launch
against torch on the inputs it read, plus the loss, and the Adam update / running statistics of the SAME step in float64
arithmetic from the gradients the step produced.  End to end against autograd carrying the same rounding points the
loss and predictions agree as at B = 6 (the stored tensors in bulk only: the network stays chaotic under storage rounding).
"""
import numpy as np
import pytest
import torch

from oracle.bf16_emulation import bf16_storage, round_bf16
from oracle.models import load_pretrained
from tests.test_gpu_train import make_batch, torch_step
from tests.test_gpu_train_bf16 import (assert_differences_sit_on_rounding_boundaries, check_adam_and_running_statistics,
                                      check_every_kernel, is_bf16)
from volpick_amd import PhaseNet
from volpick_amd.train import PhaseNetTrainer

pytestmark = [pytest.mark.gpu, pytest.mark.slow]


def _one_step(B, dtype, seed):
    x, y = make_batch(B, seed)
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B, dtype=dtype)
    w0 = tr.weights()
    loss = tr.step(x, y, lr=1e-3, update=True)  # gradients, Adam and running statistics of ONE launch sequence
    out = dict(B=B, x=x, y=y, tr=tr, loss=loss, t=tr.tensors(B), g=tr.gradients(), pred=tr.predictions(B), w0=w0, w1=tr.weights(),
               mv=tr.adam_state())
    return out


@pytest.fixture(scope="module", params=[128, 512])
def big(request):
    s = _one_step(request.param, "bf16", 1005 + request.param)
    yield s
    s["tr"].close()


def test_every_kernel_of_the_large_batch_step(big):
    s = big
    assert all(is_bf16(a) for a in (s["t"]["x"], s["t"]["inc.z"], s["t"]["up3.same.gz"]))
    # the step updated the weights AFTER its gradients were taken: the torch side must use the weights the kernels read
    net = load_pretrained("phasenet")
    sd = {k: torch.from_numpy(np.array(v)) for k, v in s["w0"].items()}
    net.load_state_dict(sd, strict=False)
    check_every_kernel(s["B"], s["x"], s["y"], s["tr"], s["loss"], s["t"], s["g"], s["pred"], net=net)


def test_adam_update_and_running_statistics_of_the_same_step(big):
    s = big
    check_adam_and_running_statistics(s["g"], s["w0"], s["w1"], s["mv"], s["t"])


def test_end_to_end_against_autograd_with_the_same_rounding_points(big):
    s = big
    net0 = load_pretrained("phasenet")
    net0.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in s["w0"].items()}, strict=False)
    with bf16_storage(net0) as net:
        want_loss, grads, z, gz, want_pred = torch_step(net, s["x"], s["y"])
    assert abs(s["loss"] - want_loss) < 1e-3 * want_loss, (s["loss"], want_loss)
    d = np.abs(s["pred"] - want_pred)
    assert np.median(d) < 1e-4 and np.percentile(d, 99) < 5e-3, (np.median(d), np.percentile(d, 99))
    # the first conv reads identical inputs on both sides: the stored bf16 values may differ only where the unrounded sum sits on a
    # rounding boundary (the bf16-MFMA form adds its exact products in another order than torch's conv) or nearly cancels
    diff = s["t"]["inc.z"] != z["inc"]
    assert diff.mean() < 0.02, diff.mean()
    ref = load_pretrained("phasenet")
    ref.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in s["w0"].items()}, strict=False)
    assert_differences_sit_on_rounding_boundaries(ref.inc, round_bf16(torch.from_numpy(s["x"])), diff, s["t"]["inc.z"], "inc.z")
    # bulk agreement of every stored tensor, as at B = 6 (tests/test_gpu_train_bf16.py): with the released weights the network is
    # chaotic under storage rounding -- one bf16 ulp in a thin BatchNorm channel flips ReLU gates downstream, so single elements
    # (and with them whole weight gradients, which sum over them) diverge between two correct implementations; the sharp check
    # is the layer-by-layer one above
    for name in z:
        e = np.abs(s["t"][name + ".z"] - z[name]) / np.abs(z[name]).max()
        assert np.median(e) < 2e-3 and np.percentile(e, 99) < 3e-2, (name, np.median(e), np.percentile(e, 99))
        e = np.abs(s["t"][name + ".gz"] - gz[name]) / np.abs(gz[name]).max()
        assert np.median(e) < 5e-3 and np.percentile(e, 99) < 1e-1, (name + ".gz", np.median(e), np.percentile(e, 99))


def test_fp32_step_past_the_switch_matches_autograd():
    """The fp32 form of the same kernels at B = 128 against plain autograd (no storage rounding: tolerances of the B = 6
    test, tests/test_gpu_train.py)."""
    B = 128
    x, y = make_batch(B, 77)
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B)
    loss = tr.step(x, y, lr=0.0, update=False)
    want_loss, grads, z, gz, pred = torch_step(load_pretrained("phasenet"), x, y)
    assert abs(loss - want_loss) < 2e-6 * max(1.0, abs(want_loss)), (loss, want_loss)
    assert np.abs(tr.predictions(B) - pred).max() < 2e-5
    t, g = tr.tensors(B), tr.gradients()
    # forward tensors end to end at the B = 6 tolerance.  The backward chain is compared KERNEL BY KERNEL on the tensors each
    # launch read (as in the bf16 form): end to end, single elements of gz whose pre-activation sits within rounding of zero
    # take the other side of the ReLU gate (the kernel gates on fma(z, scale, shift), torch on its own BatchNorm formula) --
    # 1.2e-2 of the maximum for the worst element of down3.same.gz, 6e-3 for the weight gradient that sums over it
    for name in z:
        e = float(np.abs(t[name + ".z"] - z[name]).max() / max(np.abs(z[name]).max(), 1e-30))
        assert e < 5e-4, (name + ".z", e)
        eg = np.abs(t[name + ".gz"] - gz[name]) / max(np.abs(gz[name]).max(), 1e-30)
        assert np.percentile(eg, 99.9) < 3e-3 and eg.max() < 1e-1, (name + ".gz", float(np.percentile(eg, 99.9)), float(eg.max()))
    check_every_kernel(B, x, y, tr, loss, t, g, tr.predictions(B))
    tr.close()


def test_device_inputs_may_be_refilled_right_after_an_asynchronous_step():
    """the trainer's stream is non-blocking; `step(x_dev, y_dev, want_loss=False)` returns with the step queued.
    Refilling x / y in place on torch's stream right away must not reach the queued step (vp_train_wait_inputs_consumed:
    torch's stream waits, on the device, behind the step's last read), and dropping the only reference must not let the
    caching allocator hand the memory to someone else (record_stream)."""
    B = 64
    x, y = make_batch(B, 31)
    x2, y2 = make_batch(B, 32)
    ref = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B, dtype="bf16")
    want = ref.step(x, y, lr=0.0, update=False)
    want_g = ref.gradients()
    ref.close()
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B, dtype="bf16")
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    x2d, y2d = torch.from_numpy(x2).cuda(), torch.from_numpy(y2).cuda()
    junk = torch.full_like(xd, 1e9)
    torch.cuda.synchronize()
    for _ in range(3):  # a queue of steps in front, so that the step under test is still waiting when the refill is enqueued
        tr.step(x2d, y2d, lr=0.0, update=False, want_loss=False)
    tr.step(xd, yd, lr=0.0, update=False, want_loss=False)
    xd.copy_(junk)  # in-place refill on torch's stream
    yd.copy_(junk)
    del xd, yd
    spoil = [torch.full((B, 3, 3001), 7e8, device="cuda") for _ in range(4)]  # would land in the freed blocks
    tr.synchronize()
    got_g = tr.gradients()
    for k in want_g:
        assert np.abs(got_g[k] - want_g[k]).max() <= 1e-5 * np.abs(want_g[k]).max() + 1e-12, k  # (1e9 junk would be off by 1e9)
    assert np.isfinite(want) and len(spoil) == 4
    tr.close()


def test_the_library_tells_which_queued_steps_have_read_their_inputs():
    """Round 5: the trainer object no longer records an event of its own in the trainer's stream per step; the library keeps
    a ring of events behind each step's last read of x / y (`vp_train_inputs_consumed_upto`, `vp_train_steps_enqueued`).
    Steps are numbered from 0; nothing is reported before it has completed; after a host wait everything is; the Python
    object drops the device batches it kept alive accordingly, and a fresh tensor that the allocator places where the previous
    batch lay is not mistaken for it (the producer wait is skipped only on the caller's explicit promise `inputs_unchanged=True`, never inferred)."""
    B = 64
    x, y = make_batch(B, 41)
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=B, dtype="bf16")
    lib, h = tr._lib, tr._h
    assert lib.vp_train_steps_enqueued(h) == 0 and lib.vp_train_inputs_consumed_upto(h) == -1
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    n = 12  # more than the ring holds
    for i in range(n):
        tr.step(xd, yd, lr=0.0, update=False, want_loss=False)
        assert lib.vp_train_steps_enqueued(h) == i + 1
        assert -1 <= lib.vp_train_inputs_consumed_upto(h) <= i
        assert all(seq <= i for seq, _, _ in tr._in_flight)
    tr.synchronize()
    assert lib.vp_train_inputs_consumed_upto(h) == n - 1 and not tr._in_flight
    # host batches are staged by the library: they count as steps but keep nothing alive
    tr.step(x, y, lr=0.0, update=False)
    assert lib.vp_train_steps_enqueued(h) == n + 1 and not tr._in_flight
    # a NEW pair of tensors (whatever their addresses) is waited for: results as from host arrays
    want = tr.step(x, y, lr=0.0, update=False)
    for seed in (42, 43):
        x2, y2 = make_batch(B, seed)
        ref = tr.step(x2, y2, lr=0.0, update=False)
        del xd, yd
        xd, yd = torch.from_numpy(x2).cuda(), torch.from_numpy(y2).cuda()  # may land on the freed blocks
        got = tr.step(xd, yd, lr=0.0, update=False)
        assert got == pytest.approx(ref, rel=1e-6)
    assert np.isfinite(want)
    # a refill that torch's version counter does not see (x.data.copy_): without the caller's promise the step waits for it
    x3, y3 = make_batch(B, 44)
    ref = tr.step(x3, y3, lr=0.0, update=False)
    v0 = (xd._version, yd._version)
    xd.data.copy_(torch.from_numpy(x3), non_blocking=True), yd.data.copy_(torch.from_numpy(y3), non_blocking=True)
    assert (xd._version, yd._version) == v0
    assert tr.step(xd, yd, lr=0.0, update=False) == pytest.approx(ref, rel=1e-6)
    # ... and with the promise kept (nothing written in between) the shortcut gives the same numbers
    assert tr.step(xd, yd, lr=0.0, update=False, inputs_unchanged=True) == pytest.approx(ref, rel=1e-6)
    tr.close()
