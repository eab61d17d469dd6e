"""CPU: generate.SteeredPlanner -- SteeredWindow(windowlen=in_samples, strategy="pad") as plan rows and window borders."""
from types import SimpleNamespace

import numpy as np
import pytest

from volpick_amd import generate as G

T = 3001


def cut(trace, row, in_samples):
    """The plan-row definition: x[t] = trace[start + t] where lo <= start + t < hi, else 0."""
    x = np.zeros(in_samples, trace.dtype)
    i = row["start"] + np.arange(in_samples)
    ok = (i >= row["lo"]) & (i < row["hi"])
    x[ok] = trace[i[ok]]
    return x


def plan(lengths, targets, in_samples=T):
    bank = SimpleNamespace(lengths=np.asarray(lengths, np.int64))
    t = np.asarray(targets, np.int64).reshape(-1, 3)
    return G.SteeredPlanner(bank, in_samples).plan({"trace": t[:, 0], "start_sample": t[:, 1], "end_sample": t[:, 2]})


def check_rows(lengths, targets, rows, borders, in_samples=T):
    """Each window holds the target's samples at the returned border, and zeros only where the trace has none."""
    assert rows.dtype == G.PLAN_ROW and borders.dtype == np.int32 and borders.shape == (len(targets), 2)
    for (tr, start, end), row, (a, e) in zip(targets, rows, borders):
        trace = 1 + np.arange(lengths[tr], dtype=np.int64)  # sample i holds i + 1: a zero is a pad
        x = cut(trace, row, in_samples)
        assert 0 <= a < e <= in_samples
        assert np.array_equal(x[a:e], 1 + np.arange(start, end))
        assert row["trace"] == tr and row["reserved"] == 0 and row["lo"] == 0 and row["hi"] == lengths[tr]
        n_data = min(lengths[tr], in_samples)
        assert (x != 0).sum() == n_data and (x[:n_data] != 0).all()  # zeros only behind a short trace


def test_placement_cases():
    lengths = [9000, 9000, 2000, 3001, 3002]
    targets = [
        (0, 4000, 5000),   # shorter than the window, odd remainder: (3001 - 1000) // 2 = 1000 in front, 1001 behind
        (0, 4000, 4999),   # even remainder: 1001 on either side
        (0, 4000, 5001),   # even remainder with an odd width
        (1, 3000, 6001),   # as long as the window
        (0, 0, 1000),      # at the trace start: clamps to 0
        (0, 100, 1100),    # near the start: still clamps to 0
        (1, 8000, 9000),   # at the trace end: clamps to L - T
        (1, 8999, 9000),   # one sample at the very end
        (2, 500, 1500),    # a trace shorter than T: padded, borders unchanged
        (2, 0, 2000),      # all of a short trace
        (3, 0, 3001),      # a trace exactly as long as the window
        (4, 1, 3002),      # one sample longer
    ]
    rows, borders = plan(lengths, targets)
    check_rows(lengths, targets, rows, borders)
    assert rows["start"].tolist() == [3000, 2999, 3000, 3000, 0, 0, 5999, 5999, 0, 0, 0, 1]
    assert borders.tolist() == [[1000, 2000], [1001, 2000], [1000, 2001], [0, 3001], [0, 1000], [100, 1100], [2001, 3001],
                                [3000, 3001], [500, 1500], [0, 2000], [0, 3001], [0, 3001]]


def test_the_rule_on_random_targets():
    """p0 = start - (T - (end - start)) // 2 clamped to [0, L - T], 0 on a short trace; borders (start - p0, end - p0)."""
    rng = np.random.default_rng(0)
    for in_samples in (3001, 6000):
        lengths = rng.integers(1000, 20000, 50)
        tr = rng.integers(0, 50, 400)
        L = lengths[tr]
        w = np.minimum(rng.integers(1, in_samples + 1, 400), L)
        start = (rng.random(400) * (L - w + 1)).astype(np.int64)
        targets = list(zip(tr.tolist(), start.tolist(), (start + w).tolist()))
        rows, borders = plan(lengths, targets, in_samples)
        check_rows(lengths, targets, rows, borders, in_samples)
        p0 = np.clip(start - (in_samples - w) // 2, 0, np.maximum(L - in_samples, 0))
        assert np.array_equal(rows["start"], p0)
        assert np.array_equal(borders, np.stack([start - p0, start + w - p0], 1))


def test_a_dataframe_of_targets_in_order():
    pd = pytest.importorskip("pandas")
    df = pd.DataFrame({"trace": [1, 0], "start_sample": [10, 5000], "end_sample": [1010, 8001], "phase_label": ["P", "S"]})
    rows, borders = G.SteeredPlanner(SimpleNamespace(lengths=[9000, 4000]), T).plan(df)
    assert rows["trace"].tolist() == [1, 0] and rows["hi"].tolist() == [4000, 9000]
    assert borders.tolist() == [[10, 1010], [0, 3001]]


@pytest.mark.parametrize("target,what", [
    ((0, 1000, 4002), "longer"),        # longer than the window
    ((0, 10, 10), "empty"),
    ((0, 20, 10), "empty"),
    ((0, -5, 100), "before"),
    ((0, 8500, 9001), "behind"),        # past the trace end
    ((1, 1500, 3002), "longer|behind"),  # a short trace holds borders up to T only
    ((2, 0, 10), "trace"),
])
def test_refusals(target, what):
    with pytest.raises(ValueError, match=what):
        plan([9000, 2000], [target])


def test_a_border_on_the_pad_of_a_short_trace_is_kept():
    rows, borders = plan([2000], [(0, 1500, 3001)])
    assert rows["start"].tolist() == [0] and borders.tolist() == [[1500, 3001]]
