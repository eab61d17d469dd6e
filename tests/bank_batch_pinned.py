"""What tests/test_gpu_bank_batch_pinned.py and tools/record_bank_batch_digests.py share: the bank, the rows, the conditions
the rows must meet, and the runs whose output bits are pinned (sha256 of x and y of every generator of csrc/batchgen.hip).

The fixtures are recorded from the library *before* a change of the generation code; the test then holds the library after
it to the same bits.  Rows live in tests/golden/bank_batch_rows.npz (the test does not depend on a random generator for
them), digests in tests/golden/bank_batch_digests.json."""
import ctypes as C
import hashlib
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from volpick_amd import _lib
from volpick_amd import generate as G
from volpick_amd.synthetic import synthetic_stream_array

GOLDEN = Path(__file__).resolve().parent / "golden"
ROWS_FILE, DIGEST_FILE = GOLDEN / "bank_batch_rows.npz", GOLDEN / "bank_batch_digests.json"

B = 16
SIGMA = 20.0
NORMS = ("peak", "std")
N_TRACES = 14
CONST_TRACE, NO_S_TRACE, NO_PICK_TRACE = 2, 5, 7  # channel 2 constant zero; no S onset; no onset at all
# generator -> its T values.  "windows" runs through a handle's prediction pass (vp_predict_bank), whose T is the network's
# in_samples: 3001 is the one T of the issue's list that a handle has.
CASES = {
    "windows": (3001,),
    "psn": (1, 1025, 3001, 6144),
    "det": (1, 1025, 3001, 6144),
    "psn_aug": (1, 1025, 3001, 3072),
    "det_aug": (1, 1025, 3073, 6000, 6144),
}
TRAIN_B = 4


def build_bank_arrays():
    """14 traces of unequal lengths from volpick_amd.synthetic at fixed seeds, one event each: (traces, onsets (N, 4))."""
    traces, onsets = [], []
    for i in range(N_TRACES):
        L = 9000 + 357 * i
        x, p, s = synthetic_stream_array(L, seed=4100 + i, n_events=1)
        x = x * np.float32(0.5 + 3 * i)
        ons = [float(p[0]), np.nan, float(s[0]) + 0.25, np.nan]
        if i == CONST_TRACE:
            x[2] = 0.0
        if i == NO_S_TRACE:
            ons[2] = np.nan
        if i == NO_PICK_TRACE:
            ons = [np.nan] * 4
        traces.append(np.ascontiguousarray(x, np.float32))
        onsets.append(ons)
    return traces, np.array(onsets)


def make_bank():
    traces, onsets = build_bank_arrays()
    return G.WaveformBank(traces, {"P": onsets[:, :2], "S": onsets[:, 2:]})


def aug_rows(T, lengths, onsets):
    """B hand-made vp_aug_row records at window length T that meet check_aug_rows."""
    def row(tr, start):
        return (tr, 0, int(start), 0, int(lengths[tr]))

    def at(tr, frac=4):  # a window of trace tr with its P onset (or the trace's middle) T // frac behind the start
        p = onsets[tr, 0]
        return row(tr, (int(p) if np.isfinite(p) else lengths[tr] // 2) - T // frac)

    none = (0, 0, 0, 0, 0)
    d = max(T // 3, 1)
    t = np.zeros(B, G.AUG_ROW)
    t["cut"] = T
    t[0]["primary"] = at(3)
    t[0]["event"][0] = (at(4, 5), G.AUG_BANK, T // 10, d, 0.5)
    t[1]["primary"] = at(CONST_TRACE)
    t[1]["cut"] = T - (T + 3) // 4
    t[1]["event"][0] = (row(6, lengths[6] - T // 2), G.AUG_BANK, 0, -d, 1.5)  # zero fill on the right
    t[1]["event"][1] = (at(8), G.AUG_BANK, T // 5, min(2 * d, T), 0.3)
    t[1]["noise"][0] = (row(0, 1000), G.AUG_BANK, 0.1)  # stacked noise on the primary with the constant channel
    t[2]["primary"] = at(8)
    t[2]["event"][0] = (none, G.AUG_SELF, T // 8, d, 2.0)
    t[2]["noise"][0] = (row(1, 3000), G.AUG_BANK, 0.1)
    t[2]["noise"][1] = (row(0, -(T // 2) - 1), G.AUG_BANK, 0.02)  # zero fill on the left
    t[3]["primary"] = at(NO_S_TRACE)
    t[3]["event"][0] = (at(9), G.AUG_BANK, 0, -1, 1.0)
    t[3]["gauss"], t[3]["noise_key"] = 0.1, 0x0123456789ABCDEF
    t[4]["primary"] = at(10)
    t[4]["event"][0] = (at(11), G.AUG_BANK, 0, -T, 1.0)  # wholly outside
    t[4]["gap_lo"], t[4]["gap_hi"] = T // 7, T - T // 7
    t[5]["primary"] = at(11)
    t[5]["event"][0] = (none, G.AUG_SELF, 0, 1, 0.75)
    t[5]["event"][1] = (none, G.AUG_SELF, 0, 0, 0.25)  # unshifted
    t[5]["gap_lo"], t[5]["gap_hi"] = T // 2, T // 2 + 1
    t[6]["primary"] = row(NO_PICK_TRACE, -(T // 3) - 1)
    t[6]["noise"][0] = (at(CONST_TRACE), G.AUG_BANK, 0.2)
    t[7]["primary"] = at(CONST_TRACE, 2)
    t[7]["event"][0] = (at(12), G.AUG_BANK, 0, 0, 0.8)  # a bank event with shift 0
    t[7]["noise"][0] = (row(1, 100), G.AUG_BANK, 0.5)
    t[7]["noise"][1] = (row(0, 5000), G.AUG_BANK, 0.25)
    t[8]["primary"] = at(12)  # the null record
    t[9]["primary"] = row(13, lengths[13] - T // 2)
    t[9]["gauss"], t[9]["noise_key"] = 0.15, 0xFEDCBA9876543210
    t[9]["gap_lo"], t[9]["gap_hi"] = 0, (T + 1) // 2
    t[10]["primary"] = at(CONST_TRACE, 3)
    t[10]["cut"] = T // 2
    t[10]["noise"][0] = (row(0, 2000), G.AUG_BANK, 0.3)
    t[10]["gauss"], t[10]["noise_key"] = 0.05, 7
    t[11]["primary"] = at(4)
    t[11]["event"][0] = (at(NO_S_TRACE), G.AUG_BANK, T // 6, -(T // 5), 1.2)
    t[11]["event"][1] = (none, G.AUG_SELF, T // 9, T // 4, 0.6)
    t[12]["primary"] = at(9, 2)
    t[12]["event"][0] = (at(NO_PICK_TRACE), G.AUG_BANK, 0, d, 1.0)  # a source without onsets
    t[12]["gap_lo"], t[12]["gap_hi"] = T - 1, T
    t[13]["primary"] = at(6)
    t[13]["event"][0] = (none, G.AUG_SELF, 0, T, 1.0)  # wholly outside
    t[13]["noise"][0] = (at(CONST_TRACE), G.AUG_BANK, 0.05)
    t[14]["primary"] = at(13, 6)
    t[14]["cut"] = 0
    t[14]["event"][0] = (at(3), G.AUG_BANK, T, d // 2, 0.7)  # every source sample zeroed
    t[15]["primary"] = at(0)
    t[15]["event"][0] = (at(10, 3), G.AUG_BANK, 0, T // 6, 0.9)
    t[15]["event"][1] = (at(11, 3), G.AUG_BANK, 0, T // 2, 0.4)
    t[15]["noise"][0] = (row(1, 4000), G.AUG_BANK, 0.04)
    t[15]["noise"][1] = (row(0, 6000), G.AUG_BANK, 0.03)
    t[15]["gap_lo"], t[15]["gap_hi"] = T // 3, T // 3 + T // 10
    return t


def check_aug_rows(rows, T):
    """The conditions every augmented case meets, asserted from the rows alone."""
    assert rows.dtype == G.AUG_ROW and len(rows) == B
    ev, nz = rows["event"], rows["noise"]
    used = [rows["primary"]] + [ev["row"][:, i][ev["kind"][:, i] == G.AUG_BANK] for i in range(2)] + \
           [nz["row"][:, j][nz["kind"][:, j] == G.AUG_BANK] for j in range(2)]
    used = np.concatenate(used)
    want = {
        "a bank event": (ev["kind"] == G.AUG_BANK).any(),
        "a self event": (ev["kind"] == G.AUG_SELF).any(),
        "two events": (ev["kind"] != G.AUG_NONE).all(1).any(),
        "an event with shift 0": ((ev["kind"] != G.AUG_NONE) & (ev["shift"] == 0)).any(),
        "one stacked noise source": ((nz["kind"] != G.AUG_NONE).sum(1) == 1).any(),
        "two stacked noise sources": ((nz["kind"] != G.AUG_NONE).sum(1) == 2).any(),
        "Gaussian noise": (rows["gauss"] > 0).any(),
        "a non-empty gap": (rows["gap_hi"] > rows["gap_lo"]).any(),
        "cut < T": (rows["cut"] < T).any(),
        "zero fill on the left": (used["start"] < used["lo"]).any(),
        "zero fill on the right": (used["start"] + T > used["hi"]).any(),
        "stacked noise on the constant channel": ((nz["kind"] != G.AUG_NONE).any(1) & (rows["primary"]["trace"] == CONST_TRACE)).any(),
    }
    missing = [k for k, v in want.items() if not v]
    assert not missing, (T, missing)


def check_bank(traces, onsets):
    assert len(traces) >= 12 and len({x.shape[1] for x in traces}) == len(traces)
    assert not traces[CONST_TRACE][2].any() and traces[CONST_TRACE][0].any()
    assert np.isfinite(onsets[NO_S_TRACE, 0]) and not np.isfinite(onsets[NO_S_TRACE, 2:]).any()
    assert not np.isfinite(onsets[NO_PICK_TRACE]).any()


def all_rows():
    """{"aug_T<T>": AUG_ROW records} for every T of every generator (a block-1 case runs the records' primaries)."""
    traces, onsets = build_bank_arrays()
    lengths = [x.shape[1] for x in traces]
    return {f"aug_T{T}": aug_rows(T, lengths, onsets) for T in sorted({T for ts in CASES.values() for T in ts})}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run_case(bank, gen, T, norm, rows):
    """The digest of generator `gen` at window length T on `rows` (the AUG_ROW records of T)."""
    import torch

    prim = np.ascontiguousarray(rows["primary"])
    if gen == "psn":
        out = bank.make_batch(prim, SimpleNamespace(in_samples=T, labels="PSN", norm=norm), SIGMA)
        return sha(out["X"], out["y"])
    if gen == "psn_aug":
        out = bank.make_batch(rows, SimpleNamespace(in_samples=T, labels="NPS", norm=norm), SIGMA)
        return sha(out["X"], out["y"])
    eqt = SimpleNamespace(in_samples=T, labels=["Detection", "P", "S"], norm=norm)
    if gen == "det":
        out = bank.make_batch(prim, eqt, SIGMA)
    else:
        assert gen == "det_aug"
        out = bank.make_batch_eqt_aug(rows, eqt, SIGMA, detection_fixed_window=1000 if T == 6000 else None)
    torch.cuda.synchronize()
    return sha(out["X"], out["detections"], out["y"])


def run_windows(bank, model, norm, rows):
    """The window-only generator through a one-batch prediction pass: the digest of its records and of the probabilities
    (the forward pass in between is not part of what changes; it is deterministic)."""
    import torch

    from volpick_amd import evaluate as E

    model.norm = norm
    *scores, preds = E.predict_bank(model, bank, np.ascontiguousarray(rows["primary"]), None, batch_size=B, predictions=True)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for a in scores:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest() + ":" + sha(*preds)


def run_train_step(bank, rows):
    """One vp_train_step_bank_aug step at B = 4: (loss, sha256 of the weights afterwards)."""
    from volpick_amd import PhaseNet
    from volpick_amd.train import PhaseNetTrainer

    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=TRAIN_B, device=bank.device)
    try:
        loss = tr.step_bank(bank, np.ascontiguousarray(rows[:TRAIN_B]), 1e-3, SIGMA)
        tr.synchronize()
        return loss, hashlib.sha256(tr._read(0).tobytes()).hexdigest()
    finally:
        tr.close()


def run_all(rows_by_T):
    """{case id: digest} for every pinned case, on one bank."""
    from volpick_amd import PhaseNet

    traces, onsets = build_bank_arrays()
    check_bank(traces, onsets)
    bank = make_bank()
    out = {}
    try:
        for gen, Ts in CASES.items():
            for T in Ts:
                rows = rows_by_T[f"aug_T{T}"]
                if gen.endswith("_aug"):
                    check_aug_rows(rows, T)
                for norm in NORMS:
                    if gen == "windows":
                        model = PhaseNet.from_pretrained("volpick").cuda(bank.device)
                        out[f"{gen}/T{T}/{norm}"] = run_windows(bank, model, norm, rows)
                    else:
                        out[f"{gen}/T{T}/{norm}"] = run_case(bank, gen, T, norm, rows)
        loss, wsha = run_train_step(bank, rows_by_T["aug_T3001"])
        out["train_step_bank_aug/B4/loss"] = float(loss).hex()
        out["train_step_bank_aug/B4/weights"] = wsha
    finally:
        bank.close()
    return out
