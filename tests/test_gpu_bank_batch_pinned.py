"""GPU: every batch generator of csrc/batchgen.hip writes the bits it wrote when the fixtures were recorded
(tools/record_bank_batch_digests.py, from the library before the generators were folded into one descriptor and shared
kernels): sha256 of x and y at B = 16, both norms, at the window lengths where the kernels' tiling changes; one prediction
pass for the label-free generator; and one vp_train_step_bank_aug step.  The rows and what they must contain are in
tests/bank_batch_pinned.py; the conditions are asserted on the CPU before anything runs."""
import json

import numpy as np
import pytest

from tests import bank_batch_pinned as P
from volpick_amd import generate as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    out = {k: v.view(G.AUG_ROW) for k, v in np.load(P.ROWS_FILE).items()}
    traces, onsets = P.build_bank_arrays()
    P.check_bank(traces, onsets)
    for gen, Ts in P.CASES.items():
        for T in Ts:
            assert len(out[f"aug_T{T}"]) == P.B
            if gen.endswith("_aug"):
                P.check_aug_rows(out[f"aug_T{T}"], T)
    return out


@pytest.fixture(scope="module")
def want():
    return json.loads(P.DIGEST_FILE.read_text())


@pytest.fixture(scope="module")
def bank(rows):
    bank = P.make_bank()
    yield bank
    bank.close()


@pytest.mark.parametrize("gen", [g for g in P.CASES if g != "windows"])
def test_generator_bits(bank, rows, want, gen):
    bad = []
    for T in P.CASES[gen]:
        for norm in P.NORMS:
            key = f"{gen}/T{T}/{norm}"
            if P.run_case(bank, gen, T, norm, rows[f"aug_T{T}"]) != want[key]:
                bad.append(key)
    assert not bad, bad


def test_window_only_bits_through_a_prediction_pass(bank, rows, want):
    from volpick_amd import PhaseNet

    model = PhaseNet.from_pretrained("volpick").cuda(bank.device)
    for T in P.CASES["windows"]:
        assert T == model.in_samples
        for norm in P.NORMS:
            assert P.run_windows(bank, model, norm, rows[f"aug_T{T}"]) == want[f"windows/T{T}/{norm}"], norm


def test_train_step_bank_aug_bits(bank, rows, want):
    loss, weights = P.run_train_step(bank, rows["aug_T3001"])
    assert float(loss).hex() == want["train_step_bank_aug/B4/loss"]
    assert weights == want["train_step_bank_aug/B4/weights"]
