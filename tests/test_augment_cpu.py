"""CPU: the augmented-window planner (volpick_amd/generate.py, AugmentedPlanner) against the float64 restatement of the
reference's procedure (tests/augment_restate.py) replaying the planner's own draws, its branch frequencies, subsets,
determinism and speed, and the AUG_ROW layout."""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest

from volpick_amd import _lib
from volpick_amd import generate as G
from tests import augment_restate as R

T, SIGMA = 3001, 20


def synthetic_bank(n=400, seed=0):
    """Lengths 2000-20000 and onsets of every kind: none, one, two or four, near each other or far apart."""
    rng = np.random.default_rng(seed)
    L = rng.integers(2000, 20000, n)
    ons = np.full((n, 4), np.nan)
    kind = np.arange(n) % 5
    p = rng.uniform(0, 1, n) * L
    ons[kind >= 1, 0] = p[kind >= 1]
    ons[kind >= 2, 2] = p[kind >= 2] + rng.uniform(50, 900, n)[kind >= 2]
    ons[kind == 3, 1] = p[kind == 3] + rng.uniform(2000, 4000, (kind == 3).sum())
    ons[kind == 3, 3] = ons[kind == 3, 1] + 300.5
    ons[kind == 4, 0] = p[kind == 4] + 0.5  # half-sample onsets: ties between two samples
    return SimpleNamespace(lengths=L, onsets=ons)


PROBS = {
    "reference": {},
    "superimpose": dict(event_prob=(1, 0, 0), noise_prob=(0, 0, 1), gap_prob=(0, 1)),
    "duplicate": dict(event_prob=(0, 1, 0), noise_prob=(0, 0, 1), gap_prob=(0, 1)),
    "noise": dict(event_prob=(0, 0, 1), noise_prob=(1, 0, 0), gap_prob=(1, 0)),
    "gauss": dict(event_prob=(0, 0, 1), noise_prob=(0, 1, 0), gap_prob=(0, 1)),
    "two_events": dict(event_prob=(1, 1, 0), prob_num_events={2: 1.0}),
}


def replay(planner, rows, bank, ev, nz, kw):
    for b in range(len(rows)):
        want = R.decide(rows[b]["primary"], bank.onsets, ev, nz, T, SIGMA, R.Replay(planner.last_draws, b),
                        event_prob=kw.get("event_prob", (0.2, 0.2, 0.6)), noise_prob=kw.get("noise_prob", (0.25, 0.25, 0.5)),
                        gap_prob=kw.get("gap_prob", (0.2, 0.8)),
                        num=(0.0, 1.0) if kw.get("prob_num_events") == {2: 1.0} else (0.7, 0.3))
        got = rows[b]
        assert got.tobytes() == want.tobytes(), (b, got, want)


@pytest.mark.parametrize("case", list(PROBS))
def test_planner_replays_the_restated_procedure(case):
    bank = synthetic_bank()
    ev, nz = np.arange(0, 300), np.arange(300, 400)
    kw = PROBS[case]
    planner = G.AugmentedPlanner(bank, 64, ev, nz, seed=3, sigma=SIGMA, **kw)
    for _ in range(3):
        rows = planner.plan(np.random.default_rng(1).integers(0, 400, 256))
        replay(planner, rows, bank, ev, nz, kw)


def test_replay_covers_the_edge_cases():
    """Across the reference's probabilities: truncation without an event, skipped sources, two events with e advancing,
    shifts of both signs, onsets outside the window, negative ends."""
    bank = synthetic_bank(800, seed=5)
    ev, nz = np.arange(0, 600), np.arange(600, 800)
    kw = dict(event_prob=(1, 1, 0), prob_num_events={2: 1.0})
    planner = G.AugmentedPlanner(bank, 64, ev, nz, seed=11, sigma=SIGMA, **kw)
    seen = dict(cut_only=0, skip=0, two=0, left=0, right=0, outside=0)
    for k in range(6):
        rows = planner.plan(np.arange(800)[k % 2::2])
        replay(planner, rows, bank, ev, nz, kw)
        kinds, d = rows["event"]["kind"], rows["event"]["shift"]
        seen["cut_only"] += ((rows["cut"] < T) & (kinds == 0).all(axis=1)).sum()
        seen["skip"] += ((kinds[:, 0] == 0) & (kinds[:, 1] != 0)).sum()
        seen["two"] += (kinds != 0).all(axis=1).sum()
        seen["left"] += ((kinds != 0) & (d < 0)).sum()
        seen["right"] += ((kinds != 0) & (d > 0)).sum()
        o = bank.onsets[rows["primary"]["trace"]] - rows["primary"]["start"][:, None]
        seen["outside"] += ((o < 0) | (o >= T)).any(axis=1).sum()
    assert all(v > 0 for v in seen.values()), seen


def test_zero_shift_and_skipped_source_replay():
    """Hand-made onsets: a source whose P label peaks outside its window is skipped; a shift of zero."""
    n = 4
    bank = SimpleNamespace(lengths=np.full(n, 12000), onsets=np.array([[3000.0, np.nan, 3400.0, np.nan],
                                                                         [np.nan, np.nan, 5000.0, np.nan],
                                                                         [1400.0, np.nan, np.nan, np.nan],
                                                                         [900.0, np.nan, 1200.0, np.nan]]))
    planner = G.AugmentedPlanner(bank, 4, [1], [], seed=0, sigma=SIGMA, event_prob=(1, 0, 0))
    rows = planner.plan([0, 0, 0, 0])
    assert (rows["event"]["kind"] == 0).all()  # trace 1 has no P: every source is skipped
    replay(planner, rows, bank, [1], [], dict(event_prob=(1, 0, 0)))
    # a = argmax of the source's P: q = a gives a shift of zero
    _, a = G._phase_peak(np.array([[1400.0 - 0.0, np.nan]]), np.array([0]), np.array([T]), 2.0 * SIGMA ** 2)
    assert a[0] == 1400
    assert G._shifted_argmax(np.array([[1400.0, np.nan]]), np.array([0]), T, 800.0)[0] == 1400
    assert G._shifted_argmax(np.array([[1400.0, np.nan]]), np.array([T]), T, 800.0)[0] == 0


def test_branch_frequencies_within_binomial_bounds():
    bank = synthetic_bank(2000, seed=2)
    planner = G.AugmentedPlanner(bank, 512, np.arange(1500), np.arange(1500, 2000), seed=4, sigma=SIGMA)
    u = []
    for _ in range(8):
        planner.plan(np.arange(512))
        u.append(planner.last_draws["u"])
    u = np.concatenate(u)
    n = len(u)

    def within(count, p):
        assert abs(count - n * p) <= 4.5 * np.sqrt(n * p * (1 - p)), (count, n * p)

    eb = np.searchsorted(planner.event_cum, u[:, 0], side="right")
    within((eb == 0).sum(), 0.2)
    within((eb == 1).sum(), 0.2)
    nb = np.searchsorted(planner.noise_cum, u[:, 8], side="right")
    within((nb == 0).sum(), 0.25)
    within((nb == 1).sum(), 0.25)
    within((u[:, 1] >= 0.7).sum(), 0.3)
    rows = planner.plan(np.arange(2000))
    within_n = len(rows)
    gap = rows["gap_hi"] > rows["gap_lo"]
    assert abs(gap.sum() - 0.2 * within_n) <= 4.5 * np.sqrt(within_n * 0.16) + (rows["gap_lo"] == rows["gap_hi"]).sum()
    g = rows["gauss"] > 0
    assert abs(g.sum() - 0.25 * within_n) <= 4.5 * np.sqrt(within_n * 0.1875)
    assert (rows["noise_key"][~g] == 0).all() and (rows["noise_key"][g] != 0).all()


def test_sources_come_from_their_subsets():
    bank = synthetic_bank(1000, seed=3)
    ev, nz = np.arange(0, 1000, 3), np.arange(1, 1000, 3)
    planner = G.AugmentedPlanner(bank, 512, ev, nz, seed=9, sigma=SIGMA, event_prob=(1, 0, 0), noise_prob=(1, 0, 0))
    rows = planner.plan(np.arange(1000))
    e = rows["event"][rows["event"]["kind"] == G.AUG_BANK]["row"]["trace"]
    z = rows["noise"][rows["noise"]["kind"] == G.AUG_BANK]["row"]["trace"]
    assert len(e) and len(z)
    assert np.isin(e, ev).all() and np.isin(z, nz).all()
    ev2, nz2 = G.trace_subsets({"source_type": np.array(["earthquake", "noise", "lp", "noise"])})
    assert list(ev2) == [0, 2] and list(nz2) == [1, 3]


def test_seed_determinism():
    bank = synthetic_bank()
    a = G.AugmentedPlanner(bank, 64, np.arange(300), np.arange(300, 400), seed=7, sigma=SIGMA)
    b = G.AugmentedPlanner(bank, 64, np.arange(300), np.arange(300, 400), seed=7, sigma=SIGMA)
    c = G.AugmentedPlanner(bank, 64, np.arange(300), np.arange(300, 400), seed=8, sigma=SIGMA)
    ra, rb, rc = (np.concatenate(list(p.epoch())) for p in (a, b, c))
    assert ra.tobytes() == rb.tobytes()
    assert ra.tobytes() != rc.tobytes()


def test_primary_rows_unchanged_at_zero_probabilities():
    bank = synthetic_bank()
    kw = dict(event_prob=(0, 0, 1), noise_prob=(0, 0, 1), gap_prob=(0, 1))
    aug = G.AugmentedPlanner(bank, 64, np.arange(300), np.arange(300, 400), seed=5, sigma=SIGMA, **kw)
    ref = G.WindowPlanner(bank, 64, seed=5)
    for a, r in zip(aug.epoch(), ref.epoch()):
        assert a["primary"].tobytes() == r.tobytes()
        assert (a["cut"] == T).all() and (a["event"]["kind"] == 0).all() and (a["gauss"] == 0).all()
    for a, r in zip(aug.validation(), ref.validation()):
        assert a["primary"].tobytes() == r.tobytes()
    # selection="first" leaves the default's draws alone
    w1, w2 = G.WindowPlanner(bank, 64, seed=1), G.WindowPlanner(bank, 64, seed=1, selection="random")
    assert w1.plan(np.arange(400)).tobytes() == w2.plan(np.arange(400)).tobytes()
    f = G.WindowPlanner(bank, 64, samples_before=1500, first_windowlen=4000, first_window_prob=(1, 0), selection="first")
    rows = f.plan(np.arange(400))
    first = np.nanmin(np.where(np.isfinite(bank.onsets), bank.onsets, np.inf), axis=1)
    has = np.isfinite(first)
    assert (rows["lo"][has] == np.maximum(0, np.trunc(first[has] - 1500))).all()


def test_aug_row_layout_matches_the_c_struct():
    assert G.AUG_ROW.itemsize == C.sizeof(_lib.VpAugRow)
    for name, _ in _lib.VpAugRow._fields_:
        assert G.AUG_ROW.fields[name][1] == getattr(_lib.VpAugRow, name).offset, name
    for dt, st in ((G.AUG_EVENT, _lib.VpAugEvent), (G.AUG_NOISE, _lib.VpAugNoise)):
        assert dt.itemsize == C.sizeof(st)
        for name, _ in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset, name


def test_philox_known_answers():
    """Philox4x32-10 known-answer vectors (Salmon et al., Random123)."""
    def run(ctr, key):
        return [int(w[0]) for w in R.philox4x32_10([np.array([c], np.uint64) for c in ctr], key)]

    assert run([0, 0, 0, 0], (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert run([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    n = R.gauss_noise(12345, 20000)
    assert abs(n.mean()) < 0.02 and abs(n.std() - 1) < 0.02


def test_planner_speed():
    """A 512-window batch on one host thread (the reference's probabilities): a regression bar of 2 ms, with headroom
    for slow hosts over the 0.65 ms of LOG.md section 17."""
    bank = synthetic_bank(4000, seed=6)
    planner = G.AugmentedPlanner(bank, 512, np.arange(3000), np.arange(3000, 4000), seed=1, sigma=SIGMA)
    traces = np.arange(512)
    planner.plan(traces)
    best = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(20):
            planner.plan(traces)
        best.append((time.perf_counter() - t0) / 20)
    assert min(best) <= 2e-3, min(best)
