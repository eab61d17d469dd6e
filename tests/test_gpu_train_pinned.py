"""The PhaseNet training step, pinned bit for bit: the step has no atomics and fixed fold orders, so two steps from the
shipped weights on a fixed batch leave the same bytes every time.  tests/golden/train_step_pinned.json holds SHA-256
digests of everything the trainer can read back (tools/record_train_golden.py writes it; two recordings were identical).
A host-side change that alters a launch's arguments, order or grid shows here as the first tensor that differs."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from tests.test_gpu_train import make_batch
from volpick_amd import PhaseNet
from volpick_amd.train import PhaseNetTrainer

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "train_step_pinned.json"
# (dtype, B, max_batch, windows of an update=False step in front with EMA on, or 0)
CASES = {
    "fp32-b3": ("fp32", 3, 8, 0),        # partial weight-gradient group, GB = 1
    "bf16-b3": ("bf16", 3, 8, 0),        # the same through the bf16 kernels and the conv-left statistics
    "bf16-b5-after-b8": ("bf16", 5, 8, 8),  # buffers holding a larger step; EMA
    "bf16-b129": ("bf16", 129, 136, 0),  # level-0 grids at wg_rows_cap, BatchNorm past GB = 1, the bias sum above 64
}


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _sha_named(d):
    return _sha(*(d[k] for k in sorted(d)))


def run_case(case):
    """Digests of two lr = 1e-3 steps of `case` from the shipped weights, and the launch count of the second."""
    dtype, B, max_batch, before = CASES[case]
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=max_batch, dtype=dtype)
    try:
        if before:
            tr.enable_ema()
            tr.step(*make_batch(before, 1000 + before), lr=1e-3, update=False)
        x, y = make_batch(B, 100 + B)
        losses = [tr.step(x, y, lr=1e-3, update=True) for _ in range(2)]
        assert all(np.isfinite(losses)), losses
        m, v = tr.adam_state()
        out = {"launch_count": int(tr._lib.vp_train_launch_count(tr._h)),
               "loss": _sha(np.asarray(losses, dtype=np.float64)),
               "predictions": _sha(tr.predictions(B)),
               "tensors": {k: _sha(a)[:16] for k, a in sorted(tr.tensors(B).items())},  # (64 bits each keep the file small)
               "gradients": _sha_named(tr.gradients()), "weights": _sha_named(tr.weights()),
               "adam_m": _sha_named(m), "adam_v": _sha_named(v)}
        if before:
            out["ema_weights"] = _sha_named(tr.ema_weights())
        return out
    finally:
        tr.close()


@pytest.mark.parametrize("case", list(CASES))
def test_two_training_steps_leave_the_pinned_bytes(case):
    want = json.loads(GOLDEN.read_text())[case]
    got = run_case(case)
    differ = [k for k in want["tensors"] if got["tensors"].get(k) != want["tensors"][k]]
    assert set(got["tensors"]) == set(want["tensors"]) and not differ, f"tensors that differ (in name order): {differ[:8]}"
    assert got == want, [k for k in want if got.get(k) != want[k]]
