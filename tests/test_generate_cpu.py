"""CPU: the host planner of GPU batch generation (volpick_amd/generate.py WindowPlanner) on hand-built banks."""
from types import SimpleNamespace

import numpy as np
import pytest

from volpick_amd import generate as G


def bank(lengths, p=None, s=None):
    n = len(lengths)
    ons = np.full((n, 4), np.nan)
    for col, v in ((0, p), (2, s)):
        if v is not None:
            v = np.asarray(v, np.float64).reshape(n, -1)
            ons[:, col:col + v.shape[1]] = v
    return SimpleNamespace(lengths=np.asarray(lengths, np.int64), onsets=ons)


def test_plan_row_layout_matches_the_c_struct():
    assert G.PLAN_ROW.itemsize == 32
    assert [G.PLAN_ROW.fields[k][1] for k in ("trace", "start", "lo", "hi")] == [0, 8, 16, 24]


def test_null_branch_on_a_full_trace():
    rows = G.WindowPlanner(bank([6000] * 500), 1, first_window_prob=(0, 1), seed=1).plan(np.arange(500))
    assert rows["start"].min() >= 0 and rows["start"].max() <= 2999
    assert (rows["lo"] == 0).all() and (rows["hi"] == 6000).all()
    assert len(np.unique(rows["start"])) > 100


def test_around_a_pick_keeps_the_pick_inside():
    rows = G.WindowPlanner(bank([6000] * 500, p=[4000.0] * 500), 1, first_window_prob=(1, 0), seed=2).plan(np.arange(500))
    st = rows["start"]
    assert st.min() >= 1000 and st.max() <= 3999
    assert ((st <= 4000) & (4000 < st + 3001)).all()
    assert (rows["lo"] == 1000).all() and (rows["hi"] == 6000).all()


def test_early_pick_pads_left():
    rows = G.WindowPlanner(bank([6000] * 200, p=[500.0] * 200), 1, first_window_prob=(1, 0), seed=3).plan(np.arange(200))
    assert G.PAD_LEFT_AT_NEGATIVE_P0
    # p0 = -2500: the extent [-2500, 3500) is cut to [0, 3500), the window start keeps the negative offset
    assert (rows["lo"] == 0).all() and (rows["hi"] == 3500).all()
    assert rows["start"].min() >= -2500 and rows["start"].max() <= -2500 + 2999
    assert (rows["start"] < 0).any()


def test_p0_truncates_toward_zero():
    rows = G.WindowPlanner(bank([6000], p=[500.7]), 1, first_window_prob=(1, 0), seed=0).plan([0])
    # int(500.7 - 3000) = int(-2499.3) = -2499: the extent ends at -2499 + 6000
    assert rows["hi"][0] == 3501


def test_short_trace_pads_at_the_end():
    rows = G.WindowPlanner(bank([2000] * 20), 1, first_window_prob=(0, 1), seed=4).plan(np.arange(20))
    assert (rows["start"] == 0).all() and (rows["lo"] == 0).all() and (rows["hi"] == 2000).all()


def test_trace_without_pick_takes_the_named_fallback():
    assert G.NO_PICK_FALLBACK == "null"
    rows = G.WindowPlanner(bank([8000] * 50, p=[np.nan] * 50), 1, first_window_prob=(1, 0), seed=5).plan(np.arange(50))
    # the null branch: the whole trace is the extent
    assert (rows["lo"] == 0).all() and (rows["hi"] == 8000).all()
    assert rows["start"].min() >= 0 and rows["start"].max() <= 8000 - 3001


def test_onset_drawn_among_both_phases_and_both_columns():
    b = bank([40000] * 4000, p=np.tile([[5000.0, np.nan]], (4000, 1)), s=np.tile([[15000.0, 25000.0]], (4000, 1)))
    rows = G.WindowPlanner(b, 1, first_window_prob=(1, 0), seed=6).plan(np.arange(4000))
    lo = rows["lo"]
    counts = {o: int((lo == o - 3000).sum()) for o in (5000, 15000, 25000)}
    assert sum(counts.values()) == 4000
    for c in counts.values():  # uniform over the three finite onsets: 1333 +- 4 sigma (30)
        assert abs(c - 4000 / 3) < 4 * np.sqrt(4000 * (1 / 3) * (2 / 3))


def test_branch_frequency():
    n = 20000
    rows = G.WindowPlanner(bank([20000] * n, p=[10000.0] * n), 1, seed=7).plan(np.arange(n))
    around = rows["lo"] == 7000
    assert (around | (rows["lo"] == 0)).all()
    p = 2 / 3
    assert abs(around.mean() - p) < 4 * np.sqrt(p * (1 - p) / n)


def test_sample_boundaries():
    rows = G.WindowPlanner(bank([20000] * 300), 1, first_window_prob=(0, 1), sample_boundaries=(1000, 5000),
                           seed=8).plan(np.arange(300))
    assert rows["start"].min() >= 1000 and rows["start"].max() <= 5000 - 3001


def test_seed_determines_the_plans():
    b = bank(np.arange(100) * 50 + 2500, p=np.linspace(100, 7000, 100), s=np.linspace(900, 7900, 100))
    a1 = G.WindowPlanner(b, 8, seed=11).plan(np.arange(100))
    a2 = G.WindowPlanner(b, 8, seed=11).plan(np.arange(100))
    a3 = G.WindowPlanner(b, 8, seed=12).plan(np.arange(100))
    assert (a1 == a2).all()
    assert not (a1 == a3).all()


def test_epochs_are_permutations_with_drop_last():
    pl = G.WindowPlanner(bank([4000] * 23), 5, seed=9)
    epochs = [[r["trace"].copy() for r in pl.epoch()] for _ in range(3)]
    for ep in epochs:
        assert [len(b) for b in ep] == [5, 5, 5, 5]
        seen = np.concatenate(ep)
        assert len(np.unique(seen)) == 20 and seen.max() < 23
    assert not all((np.concatenate(epochs[0]) == np.concatenate(e)).all() for e in epochs[1:])


def test_validation_keeps_order_and_the_last_partial_batch():
    pl = G.WindowPlanner(bank([4000] * 23), 5, seed=10)
    batches = list(pl.validation())
    assert [len(b) for b in batches] == [5, 5, 5, 5, 3]
    assert (np.concatenate([b["trace"] for b in batches]) == np.arange(23)).all()


def test_label_rows_and_row_conversion():
    assert G.label_rows("PSN").tolist() == [0, 1, 2]
    assert G.label_rows("NPS").tolist() == [1, 2, 0]
    with pytest.raises(ValueError):
        G.label_rows("PSX")
    rec = np.zeros(3, [("trace", "i8"), ("start", "i8"), ("lo", "i8"), ("hi", "i8")])
    rec["hi"] = 7
    r = G.as_rows(rec)
    assert r.dtype == G.PLAN_ROW and (r["hi"] == 7).all()


def test_onset_table_and_prob_label_shape():
    t = G._onset_table({"P": [1.0, 2.0], "S": [[3.0, 4.0], [np.nan, 5.0]]}, 2)
    assert np.array_equal(t, np.array([[1, np.nan, 3, 4], [2, np.nan, np.nan, 5]]), equal_nan=True)
    from volpick_amd.train import PhaseNetLit

    with pytest.raises(ValueError, match="gaussian"):
        PhaseNetLit(prob_label_shape="triangle")
