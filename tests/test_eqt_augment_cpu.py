"""CPU: EQTransformer's stacked recipe without a GPU.  The planner with EQTransformer's windows (EQTransformerLit.
augmented_planner) against the restated procedure replaying its own draws; its source windows; the default planner
unchanged; the float64 restatement of the record's window (tests/eqt_augment_restate.py) on hand-made records whose
rows are worked out by hand; and the two new entry points declared, exported and bound."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from volpick_amd import _lib
from volpick_amd import generate as G
from volpick_amd.train import EQTransformerLit
from tests import eqt_augment_restate as R

T, SIGMA = 6000, 20
ROOT = Path(__file__).resolve().parents[1]


def synthetic_bank(n=400, seed=0):
    """Lengths 14000-30000; onsets of every kind: none, a P alone, P and S, two of each, half-sample onsets.  The last
    quarter are the noise sources -- some of them with a pick, so that their around-a-pick windows are planned too."""
    rng = np.random.default_rng(seed)
    L = rng.integers(14000, 30000, n)
    ons = np.full((n, 4), np.nan)
    kind = np.arange(n) % 5
    p = rng.uniform(0.05, 0.8, n) * L
    ons[kind >= 1, 0] = p[kind >= 1]
    ons[kind >= 2, 2] = p[kind >= 2] + rng.uniform(50, 900, n)[kind >= 2]
    ons[kind == 3, 1] = p[kind == 3] + rng.uniform(2000, 4000, (kind == 3).sum())
    ons[kind == 3, 3] = ons[kind == 3, 1] + 300.5
    ons[kind == 4, 0] = np.floor(p[kind == 4]) + 0.5
    return SimpleNamespace(lengths=L, onsets=ons)


def eqt_planner(bank, B, seed, ev, nz, **params):
    lit = EQTransformerLit(sigma=SIGMA, model=SimpleNamespace(in_samples=T, labels=["Detection", "P", "S"], norm="std"))
    return lit.augmented_planner(bank, B, G.Augmentation(event_traces=ev, noise_traces=nz, **params), seed=seed)


def test_eqt_planner_replays_the_restated_procedure_and_takes_every_branch():
    bank = synthetic_bank()
    ev, nz = np.arange(0, 300), np.arange(300, 400)
    seen = dict(superimpose=0, duplicate=0, no_event=0, one_event=0, two_events=0, bank_event=0, self_event=0, both_events=0,
                stacked_noise=0, gauss=0, no_noise=0, one_noise=0, two_noise=0, gap=0, no_gap=0, cut=0, zero_shift_or_not=0)
    for seed in (1, 2, 3):
        planner = eqt_planner(bank, 64, seed, ev, nz)
        assert planner.T == T and planner.primary.samples_before == 6000 and planner.primary.first_windowlen == 12000
        rows = planner.plan(np.random.default_rng(seed).integers(0, 400, 256))
        for b in range(len(rows)):
            want = R.decide(rows[b]["primary"], bank.onsets, ev, nz, T, SIGMA, R.Replay(planner.last_draws, b))
            assert rows[b].tobytes() == want.tobytes(), (seed, b, rows[b], want)
        u = planner.last_draws["u"]
        eb = np.searchsorted(planner.event_cum, u[:, G.U_COLS["event_branch"]], side="right")
        nb = np.searchsorted(planner.noise_cum, u[:, G.U_COLS["noise_branch"]], side="right")
        gb = np.searchsorted(planner.gap_cum, u[:, G.U_COLS["gap_branch"]], side="right")
        kinds = rows["event"]["kind"]
        seen["superimpose"] += (eb == 0).sum()
        seen["duplicate"] += (eb == 1).sum()
        seen["no_event"] += (eb == 2).sum()
        seen["one_event"] += (u[:, G.U_COLS["n_events"]] < 0.7).sum()
        seen["two_events"] += (u[:, G.U_COLS["n_events"]] >= 0.7).sum()
        seen["bank_event"] += (kinds == G.AUG_BANK).any(axis=1).sum()
        seen["self_event"] += (kinds == G.AUG_SELF).any(axis=1).sum()
        seen["both_events"] += (kinds != 0).all(axis=1).sum()
        seen["stacked_noise"] += (nb == 0).sum()
        seen["gauss"] += ((nb == 1) & (rows["gauss"] > 0)).sum()
        seen["no_noise"] += (nb == 2).sum()
        seen["one_noise"] += ((rows["noise"]["kind"] != 0).sum(axis=1) == 1).sum()
        seen["two_noise"] += ((rows["noise"]["kind"] != 0).sum(axis=1) == 2).sum()
        seen["gap"] += ((gb == 0) & (rows["gap_hi"] > rows["gap_lo"])).sum()
        seen["no_gap"] += (gb == 1).sum()
        seen["cut"] += (rows["cut"] < T).sum()
        seen["zero_shift_or_not"] += ((kinds != 0) & (rows["event"]["shift"] != 0)).sum()
    assert all(v > 0 for v in seen.values()), seen


def test_source_windows_are_eqtransformers():
    """Event sources: an extent of 8000 samples with the first onset 3000 samples in; noise sources: the primary's block 1,
    an extent of 12000 samples with an onset 6000 samples in, or the whole trace."""
    bank = synthetic_bank(seed=4)
    ev, nz = np.arange(0, 300), np.arange(300, 400)
    planner = eqt_planner(bank, 64, 5, ev, nz, event_prob=(1, 0, 0), noise_prob=(1, 0, 0))
    planner.plan(np.arange(256))
    d = planner.last_draws
    rows, tr = d["event_rows"].ravel(), d["event_traces"].ravel()
    assert (rows["trace"] == tr).all()
    L = bank.lengths[tr]
    first = np.where(np.isfinite(bank.onsets[tr]), bank.onsets[tr], np.inf).min(axis=1)
    has = np.isfinite(first)
    assert has.sum() > 100 and (~has).sum() > 0
    p0 = np.trunc(first[has] - 3000).astype(np.int64)  # the onset stands at sample 3000 of the extent
    assert (rows["lo"][has] == np.maximum(0, p0)).all() and (rows["hi"][has] == np.minimum(L[has], p0 + 8000)).all()
    assert ((rows["start"][has] >= p0) & (rows["start"][has] <= p0 + 2000)).all() and (rows["start"][has] > p0).any()
    assert (rows["lo"][~has] == 0).all() and (rows["hi"][~has] == L[~has]).all()  # no pick: the null branch
    rows, tr = d["noise_rows"].ravel(), d["noise_traces"].ravel()
    L = bank.lengths[tr]
    null = (rows["lo"] == 0) & (rows["hi"] == L)
    around = np.zeros(len(rows), bool)
    for j in range(4):
        with np.errstate(invalid="ignore"):
            p0 = np.trunc(np.nan_to_num(bank.onsets[tr, j] - 6000)).astype(np.int64)
        ok = np.isfinite(bank.onsets[tr, j]) & (rows["lo"] == np.maximum(0, p0)) & (rows["hi"] == np.minimum(L, p0 + 12000))
        ok &= (rows["start"] >= p0) & (rows["start"] <= p0 + 6000)
        around |= ok
    assert (null | around).all() and (around & ~null).sum() > 20 and (null & ~around).sum() > 20


def test_default_arguments_keep_every_row():
    """The planner as it was built before it had the event_* and block-1 arguments: its source planners constructed the old
    way, in place, on the same generator."""
    bank = synthetic_bank(seed=7)
    ev, nz = np.arange(0, 300), np.arange(300, 400)
    kw = dict(event_prob=(1, 1, 1), noise_prob=(1, 1, 1), gap_prob=(1, 1))
    new = G.AugmentedPlanner(bank, 64, ev, nz, seed=3, sigma=SIGMA, **kw)
    old = G.AugmentedPlanner(bank, 64, ev, nz, seed=3, sigma=SIGMA, **kw)
    old.event_planner = G.WindowPlanner(bank, 64, samples_before=1500, first_windowlen=4000, first_window_prob=(1, 0),
                                        in_samples=3001, selection="first")
    old.noise_planner = G.WindowPlanner(bank, 64, in_samples=3001)
    old.event_planner.rng = old.noise_planner.rng = old.rng
    via = G.Augmentation(event_traces=ev, noise_traces=nz, **kw).planner(bank, 64, 3, sigma=SIGMA)
    for _ in range(3):
        traces = np.random.default_rng(2).integers(0, 400, 256)
        a, b, c = new.plan(traces), old.plan(traces), via.plan(traces)
        assert a.tobytes() == b.tobytes() == c.tobytes()
        assert (a["event"]["kind"] == G.AUG_BANK).any() and (a["noise"]["kind"] != 0).any()
    # and the new arguments reach the source planners
    eq = G.AugmentedPlanner(bank, 64, ev, nz, seed=3, sigma=SIGMA, event_samples_before=3000, event_windowlen=8000,
                            samples_before=6000, first_windowlen=12000, in_samples=T, **kw)
    assert (eq.event_planner.samples_before, eq.event_planner.first_windowlen) == (3000, 8000)
    assert (eq.noise_planner.samples_before, eq.noise_planner.first_windowlen) == (6000, 12000)


# ------------------------------------------------------------------------------------------------- hand-made records
@pytest.fixture(scope="module")
def hand():
    traces = R.hand_traces()
    recs, want, names = R.hand_records()
    out = [R.execute_eqt(r, traces, R.HAND_ONSETS, T, SIGMA, "peak", (0, 1, 2)) for r in recs]
    return traces, recs, want, dict(zip(names, out))


def g(t, o):
    return np.exp(-((t - o) ** 2) / (2.0 * SIGMA ** 2))


def test_hand_records_detection_rows(hand):
    assert G.DETECTION_UNSHIFTED == "dropped"
    _, recs, want, out = hand
    for name, w in zip("abcde", want):
        assert np.array_equal(out[name][1][0], w), name
    assert out["a"][1][0].sum() == 1200          # (a) shift 0: the source's box [1500, 2460) is NOT merged ...
    assert out["b"][1][0].sum() == 1461          # (b) ... shift 1: it is, as [1501, 2461)
    assert out["b"][1][0][2460] == 1 and out["b"][1][0][2461] == 0
    assert out["c"][1][0][5500:].all() and out["c"][1][0][2200:5500].sum() == 0  # (c) runs off the end
    d = out["d"][1]
    assert (d[:, 1200:1800] == 0).all() and d[0, 1199] == 1 and d[0, 1800] == 1  # (d) zeros inside, the box kept outside
    assert d[2, 1500] == 0 and d[1, 1000] == 1                                    # ... the S peak lies in the gap


def test_hand_records_phase_rows_are_maxima_without_rescaling(hand):
    _, recs, _, out = hand
    t = np.arange(T, dtype=np.float64)
    ya = out["a"][1]
    # (a) the source's P stands on the primary's S at 1500: both stay 1 (a division by max(1, P + S) would halve them)
    assert ya[1, 1000] == 1 and ya[1, 1500] == 1 and ya[2, 1500] == 1 and ya[2, 1900] == 1
    assert np.array_equal(ya[1], np.maximum(g(t, 1000), g(t, 1500))) and np.array_equal(ya[2], np.maximum(g(t, 1500), g(t, 1900)))
    yb = out["b"][1]
    assert yb[1, 1501] == 1 and yb[2, 1901] == 1 and yb[1, 1500] == g(1500, 1501)
    yc = out["c"][1]
    assert yc[1, 5500] == 1 and yc[2, 5999] == g(5999, 6000) and np.array_equal(yc[2, :3000], g(t, 1500)[:3000])
    # (e) two P Gaussians 30 samples apart: their sum exceeds 1 between them, the row is their maximum
    ye = out["e"][1]
    assert np.array_equal(ye[1], np.maximum(g(t, 1000), g(t, 1030)))
    assert ye[1, 1015] == np.exp(-225.0 / 800.0) and 2 * ye[1, 1015] > 1 and ye[1].max() == 1
    assert not ye[2, :1400].all() and np.array_equal(ye[2], g(t, 1500))  # the source has no S


def test_hand_records_waveforms(hand):
    traces, recs, _, out = hand
    # (d) the gap is constant after the second normalisation: zeros, demeaned and scaled
    xd = out["d"][0]
    assert (np.ptp(xd[:, 1200:1800], axis=1) == 0).all() and np.abs(xd).max() == pytest.approx(1.0, abs=1e-9)
    # (a) and (b) differ by the one-sample shift of the scaled source behind zero_before
    x0 = R.window(traces, recs[0]["primary"], T, "peak")
    s = R.window(traces, recs[0]["event"][0]["row"], T, "peak")
    s[:, :1300] = 0
    assert np.allclose(out["a"][0], R.normalise(x0 + 0.5 * s, "peak"), rtol=0, atol=1e-15)
    assert np.allclose(out["b"][0], R.normalise(x0 + 0.5 * R.shift(s, 1), "peak"), rtol=0, atol=1e-15)
    # (c) the duplicate: the primary's own window from zero_before on, 4500 samples later, twice as large
    s = x0.copy()
    s[:, :800] = 0
    assert np.allclose(out["c"][0], R.normalise(x0 + 2.0 * R.shift(s, 4500), "peak"), rtol=0, atol=1e-15)


# -------------------------------------------------------------------------------------------------------- the symbols
NAMES = ["vp_bank_make_batch_eqt_aug", "vp_validate_eqt_bank_aug"]


def test_symbols_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "volpick_hip.h").read_text()
    for name, like in zip(NAMES, ["vp_bank_make_batch_eqt", "vp_validate_eqt_bank"]):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert "const vp_aug_row* rows" in m.group(1) and "float det_fixed_window" in m.group(1)
        assert argtypes == _lib.SIGNATURES[like][1]  # the plan-row entry point's arguments, the rows of another type
        assert hasattr(lib, name), f"{name} is not exported"
    assert "DETECTION_UNSHIFTED" in (ROOT / "volpick_amd" / "generate.py").read_text()


def test_null_arguments_are_refused_without_a_device(lib):
    lr = (C.c_int * 3)(0, 1, 2)
    w = (C.c_double * 3)(0.05, 0.4, 0.55)
    assert lib.vp_bank_make_batch_eqt_aug(None, None, 1, T, 20.0, 0, lr, -1.0, None, None, None) == -1
    assert lib.vp_last_error() == b"vp_bank_make_batch_eqt_aug: null argument"  # (the shared bodies name their caller)
    assert lib.vp_validate_eqt_bank_aug(None, None, None, 1, 20.0, 0, lr, -1.0, w, None) == -1
    assert lib.vp_last_error() == b"vp_validate_eqt_bank_aug: null argument"
