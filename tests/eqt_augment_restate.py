"""Helper of the EQTransformer stacked-recipe tests (not a test module): a float64 numpy restatement of the window an
AUG_ROW record defines for a detection-row model (include/volpick_hip.h, vp_bank_make_batch_eqt_aug, steps 1-7), written
from that description with the pieces of tests/augment_restate.py and tests/eqt_batch_restate.py; and the hand-made
records both test files use, with the rows they must give worked out by hand."""
import numpy as np

from volpick_amd import generate as G
from tests.augment_restate import Replay, decide, gauss_noise, labels_of, normalise, shift, window  # noqa: F401
from tests.eqt_batch_restate import detection_row


def execute_eqt(rec, traces, onsets, T, sigma, norm, label_rows, fixed_window=None):
    """x, y (3, T) float64 of one AUG_ROW record; ``label_rows`` = the rows of detection, P and S in y."""
    i_det, i_p, i_s = label_rows
    pr = rec["primary"]
    x0 = window(traces, pr, T, norm)
    pons = onsets[int(pr["trace"])] - float(pr["start"])
    P, S = labels_of(pons, T, sigma)
    D0 = detection_row(pons, T, fixed_window)
    D = D0.copy()
    x = x0.copy()
    x[:, int(rec["cut"]):] = 0
    for ev in rec["event"]:
        if ev["kind"] == G.AUG_NONE:
            continue
        if ev["kind"] == G.AUG_BANK:
            s = window(traces, ev["row"], T, norm)
            s[np.all(np.abs(x) <= 1e-8, axis=1)] = 0
            sons = onsets[int(ev["row"]["trace"])] - float(ev["row"]["start"])
            Ds = detection_row(sons, T, fixed_window)
        else:
            s, sons, Ds = x0.copy(), pons, D0
        s[:, :int(ev["zero_before"])] = 0
        d = int(ev["shift"])
        x = x + float(ev["scale"]) * shift(s, d)
        P2, S2 = shift(labels_of(sons, T, sigma), d)
        P, S = np.maximum(P, P2), np.maximum(S, S2)  # noise_label=False: nothing else
        assert G.DETECTION_UNSHIFTED == "dropped"
        if d != 0:
            D = np.maximum(D, shift(Ds, d))
    for nz in rec["noise"]:
        if nz["kind"] == G.AUG_NONE:
            continue
        s = window(traces, nz["row"], T, norm)
        s[np.all(np.abs(x) <= 1e-8, axis=1)] = 0
        x = x + s * (np.abs(x).max() * float(nz["scale"]))
    if rec["gauss"] > 0:
        x = x + float(rec["gauss"]) * x.max() * gauss_noise(rec["noise_key"], T)
    g0, g1 = int(rec["gap_lo"]), int(rec["gap_hi"])
    x[:, g0:g1] = 0
    y = np.zeros((3, T))
    y[i_p], y[i_s], y[i_det] = P, S, D
    y[:, g0:g1] = 0
    return normalise(x, norm), y


# ---------------------------------------------------------------------------------------------------- hand-made records
# A bank of three traces for the records (a)-(e): the onsets are whole samples, so every box border is an integer worked
# out below.  Trace 0 (primary, from sample 0): P 1000, S 1500 -> box [1000, 1500 + 1.4 * 500) = [1000, 2200).
# Trace 1 (source): P 3000, S 3400 -> in a window that starts at 1500: P 1500, S 1900, box [1500, 1900 + 560) =
# [1500, 2460), which ends behind the primary's.  Trace 2 (source of (e)): P 4030 -> at start 3000: P 1030, 30 samples
# behind the primary's P; no S, no box.
HAND_T = 6000
HAND_L = 14000
HAND_ONSETS = np.array([[1000.0, np.nan, 1500.0, np.nan],
                        [3000.0, np.nan, 3400.0, np.nan],
                        [4030.0, np.nan, np.nan, np.nan]])


def hand_traces(seed=3):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((3, HAND_L)).astype(np.float32) * (1.0 + i) for i in range(3)]


def box(*spans, T=HAND_T):
    y = np.zeros(T)
    for lo, hi in spans:
        y[max(lo, 0):max(min(hi, T), 0)] = 1
    return y


def hand_records():
    """(records, expected detection rows, name) of the cases (a)-(e); the primary is trace 0 from sample 0."""
    recs = np.zeros(5, G.AUG_ROW)
    recs["cut"] = HAND_T
    for r in recs:
        r["primary"] = (0, 0, 0, 0, HAND_L)
    src = (1, 0, 1500, 0, HAND_L)
    # (a) a superimposed source with shift 0: P / S merged (the source's P at 1500, S at 1900), its box dropped
    recs[0]["event"][0] = (src, G.AUG_BANK, 1300, 0, 0.5)
    # (b) the same source with shift 1: its box [1500, 2460) is merged as [1501, 2461)
    recs[1]["event"][0] = (src, G.AUG_BANK, 1300, 1, 0.5)
    # (c) a duplicate whose shifted box [1000 + 4500, 2200 + 4500) runs off the end at 6000
    recs[2]["event"][0] = ((0, 0, 0, 0, 0), G.AUG_SELF, 800, 4500, 2.0)
    # (d) a gap [1200, 1800) across the primary's box: zeros inside, the box kept outside
    recs[3]["gap_lo"], recs[3]["gap_hi"] = 1200, 1800
    # (e) the P Gaussians of two events 30 samples apart overlap: y = max, no rescaling; no S, no box in the source
    recs[4]["event"][0] = ((2, 0, 3000, 0, HAND_L), G.AUG_BANK, 830, 0, 1.0)
    want = [box((1000, 2200)),
            box((1000, 2461)),
            box((1000, 2200), (5500, 6700)),
            box((1000, 1200), (1800, 2200)),
            box((1000, 2200))]
    return recs, want, ["a", "b", "c", "d", "e"]
