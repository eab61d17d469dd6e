"""CPU: the host side of task 0 (volpick_amd/evaluate.py) -- counts and residuals on cases worked by hand and against
outputs recorded from the reference's own functions, the metric table against the statistics written out in numpy, the
ground truth, the true-negative rows, the optimal-threshold summary -- and the numpy restatement of the sweep
(tests/task0_restate.py) against the oracle's ``picks_from_trace``."""
import json
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from oracle.pipeline import picks_from_trace
from tests import task0_restate as R
from volpick_amd import evaluate as E

GOLDEN = Path(__file__).resolve().parent / "golden" / "task0_reference_cases.json"


def padded(picks, start=None, K=8):
    """One threshold's pick lists (trace samples) -> count (n, 1), peak (n, 1, K) local to ``start``, start."""
    n = len(picks)
    start = np.zeros(n, np.int64) if start is None else np.asarray(start, np.int64)
    count = np.array([[len(p)] for p in picks], np.int32)
    peak = np.full((n, 1, K), -1, np.int32)
    for i, p in enumerate(picks):
        peak[i, 0, :len(p)] = np.asarray(p, np.int64) - start[i]
    return count, peak, start


# target: onset, picks                      method 0            method 1
HAND = [(100.0, [60, 149, 151]),          # TP 1, FP 1          TP 1                 (the issue's example)
        (np.nan, [5, 9]),                 # FP 2                FP 1
        (200.0, []),                      # FN 1                FN 1
        (np.nan, []),                     # nothing             nothing
        (300.0, [400]),                   # FN 1, FP 1          FP 1
        (500.0, [450, 550])]              # TP 1                TP 1: two picks equally close, both at the bound
HAND_START = [40, 0, 150, 7, 250, 449]


def test_counts_and_residuals_by_hand():
    truth = np.array([t for t, _ in HAND])
    count, peak, start = padded([p for _, p in HAND], HAND_START)
    TP, FP, FN, tps, fps, fns = E.task0_counts(truth, count, peak, start, tp_thre=0.5, method=0)
    assert (TP, FP, FN) == (2, 4, 2) and TP.shape == (1,) and tps.shape == (6, 1) and tps.dtype == np.float64
    assert tps[:, 0].tolist() == [1, 0, 0, 0, 0, 1] and fps[:, 0].tolist() == [1, 2, 0, 0, 1, 0]
    assert fns[:, 0].tolist() == [0, 0, 1, 0, 1, 0]
    res = E.task0_residuals(truth, count, peak, start, method=0)
    assert len(res) == 1 and res[0].tolist() == [-0.4, 0.49, 0.51, 1.0, -0.5, 0.5]
    TP, FP, FN, tps, fps, fns = E.task0_counts(truth, count, peak, start, tp_thre=0.5, method=1)
    assert (TP, FP, FN) == (2, 2, 1)
    assert tps[:, 0].tolist() == [1, 0, 0, 0, 0, 1] and fps[:, 0].tolist() == [0, 1, 0, 0, 1, 0]
    assert fns[:, 0].tolist() == [0, 0, 1, 0, 0, 0]
    assert E.task0_residuals(truth, count, peak, start, method=1)[0].tolist() == [-0.4, 1.0, -0.5]
    # a tighter bound: 0.4 s keeps the first target's pick at -0.4 s (<=) and drops the last target's
    TP, FP, FN, *_ = E.task0_counts(truth, count, peak, start, tp_thre=0.4, method=0)
    assert (TP, FP, FN) == (1, 7, 3)
    with pytest.raises(ValueError):
        E.task0_counts(truth, count, peak, start, method=2)
    with pytest.raises(ValueError):
        E.task0_residuals(truth, count, peak, start, method=2)


def test_counts_and_residuals_equal_the_reference_recordings():
    doc = json.loads(GOLDEN.read_text())
    assert "count_TP_FP_FN" in doc["made_by"] and len(doc["cases"]) == 48
    seen = set()
    for c in doc["cases"]:
        truth = np.array([t[0] if t else np.nan for t in c["truth"]])
        start = np.arange(len(truth)) * 3  # the picks are trace samples whatever the window's start
        count, peak, start = padded(c["picks"], start)
        got = E.task0_counts(truth, count, peak, start, c["tp_thre"], c["sampling_rate"], c["method"])
        assert [float(g[0]) for g in got[:3]] == [c["TP"], c["FP"], c["FN"]]
        for g, k in zip(got[3:], ("tps", "fps", "fns")):
            assert g[:, 0].tolist() == c[k], k
        res = E.task0_residuals(truth, count, peak, start, c["sampling_rate"], c["method"])[0]
        assert res.tolist() == c["residuals"]
        seen.add((c["method"], c["tp_thre"]))
    assert seen == {(0, 0.5), (0, 0.1), (1, 0.5), (1, 0.1)}


def stats_in_numpy(r):
    """The reference's residual statistics, spelled out (eval_taks0.py:605-641)."""
    m = r.copy()
    m[m < -1] = -1
    m[m > 1] = 1
    m2 = r[(r > -1) & (r < 1)]
    mad = lambda a: np.median(np.abs(a - np.median(a)))
    return {"mean": np.mean(r), "median": np.median(r), "std": np.std(r, ddof=1), "MAE": np.mean(np.abs(r)), "MAD": mad(r),
            "out": r[(r < -1) | (r > 1)].size / r.size,
            "modified_mean": np.mean(m), "modified_median": np.median(m), "modified_std": np.std(m, ddof=1),
            "modified_RMSE": np.sqrt(np.mean(m**2)), "modified_MAE": np.mean(np.abs(m)), "modified_MAD": mad(m),
            "modified_mean2": np.mean(m2), "modified_median2": np.median(m2), "modified_std2": np.std(m2, ddof=1),
            "modified_RMSE2": np.sqrt(np.mean(m2**2)), "modified_MAE2": np.mean(np.abs(m2)), "modified_MAD2": mad(m2)}


PHASE_KEYS = ["TP", "FP", "FN", "precision", "recall", "F1score"] + list(E.TASK0_RESIDUAL_KEYS)


def same_number(a, b):
    return (a is None and b is None) or (a is not None and b is not None and (a == b or (np.isnan(a) and np.isnan(b))))


def metric_case():
    """Three thresholds over 40 targets: many picks, P picks on one target only (one residual), and none at all."""
    rng = np.random.default_rng(8)
    n, K = 40, 8
    p_truth = np.where(rng.random(n) < 0.7, rng.integers(500, 2500, n), np.nan).astype(np.float64)
    s_truth = np.where(rng.random(n) < 0.5, rng.integers(500, 2500, n) + 0.5, np.nan)
    start = rng.integers(0, 400, n)
    count = np.zeros((n, 2, 3), np.int32)
    peak = np.full((n, 2, 3, K), -1, np.int32)
    for i in range(n):
        for ph, truth in enumerate((p_truth, s_truth)):
            k = int(rng.integers(0, 5))
            near = (0 if np.isnan(truth[i]) else truth[i]) + rng.choice([-260, -101, -100, -40, 0, 3, 50, 51, 99, 100, 180], k)
            p = np.unique(np.clip(near, start[i], None).astype(np.int64)) - start[i]
            count[i, ph, 0], peak[i, ph, 0, :len(p)] = len(p), p
    first = int(np.flatnonzero(~np.isnan(p_truth))[0])
    count[first, 0, 1], peak[first, 0, 1, 0] = 1, int(p_truth[first]) + 30 - start[first]
    return p_truth, s_truth, count, peak, start


def test_metrics_table_keys_values_and_empty_rows():
    p_truth, s_truth, count, peak, start = metric_case()
    thr = np.array([0.1, 0.5, 0.9])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rows = E.task0_metrics(p_truth, s_truth, count, peak, start, thr, tp_thre=0.5, count_tp_method=0)
    assert any(issubclass(w.category, RuntimeWarning) for w in caught)  # 0 / 0 and ddof = 1 of one value: numpy's, kept
    assert len(rows) == 3
    for j, row in enumerate(rows):
        assert list(row) == ["prob_thre", "tp_thre"] + [f"p_{k}" for k in PHASE_KEYS] + [f"s_{k}" for k in PHASE_KEYS]
        assert row["prob_thre"] == thr[j] and row["tp_thre"] == 0.5
        for ph, (name, truth) in enumerate((("p", p_truth), ("s", s_truth))):
            TP, FP, FN, *_ = E.task0_counts(truth, count[:, ph], peak[:, ph], start, 0.5, method=0)
            assert (row[f"{name}_TP"], row[f"{name}_FP"], row[f"{name}_FN"]) == (TP[j], FP[j], FN[j])
            r = E.task0_residuals(truth, count[:, ph], peak[:, ph], start, method=0)[j]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                prec, rec = TP[j] / (TP[j] + FP[j]), TP[j] / (TP[j] + FN[j])
                want = {"precision": prec, "recall": rec, "F1score": 2.0 * (prec * rec) / (prec + rec)}
                want.update(stats_in_numpy(r) if len(r) else dict.fromkeys(E.TASK0_RESIDUAL_KEYS))
            for k, v in want.items():
                assert same_number(row[f"{name}_{k}"], v), (j, name, k, row[f"{name}_{k}"], v)
    # threshold 0: residuals on both sides of +-1 s, every statistic a number
    assert rows[0]["p_out"] > 0 and all(np.isfinite(rows[0][f"p_{k}"]) for k in PHASE_KEYS)
    # threshold 1: one P residual (0.3 s): its ddof = 1 deviation is NaN, the rest are numbers; no S picks at all
    assert rows[1]["p_TP"] == 1 and rows[1]["p_mean"] == 0.3 and np.isnan(rows[1]["p_std"]) and rows[1]["p_MAD"] == 0
    assert rows[1]["s_mean"] is None and rows[1]["s_modified_MAD2"] is None and rows[1]["s_TP"] == 0
    assert np.isnan(rows[1]["s_precision"]) and rows[1]["s_recall"] == 0 and np.isnan(rows[1]["s_F1score"])
    # threshold 2: nothing picked
    assert all(rows[2][f"{n}_{k}"] is None for n in "ps" for k in E.TASK0_RESIDUAL_KEYS)
    assert rows[2]["p_FN"] == (~np.isnan(p_truth)).sum() and np.isnan(rows[2]["p_precision"])


def test_metrics_without_one_phase_and_with_method_1():
    p_truth, s_truth, count, peak, start = metric_case()
    thr = [0.1, 0.5, 0.9]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        both = E.task0_metrics(p_truth, s_truth, count, peak, start, thr, count_tp_method=1)
        only_s = E.task0_metrics(p_truth, s_truth, count, peak, start, thr, count_tp_method=1, no_p=True)
        only_p = E.task0_metrics(p_truth, s_truth, count, peak, start, thr, count_tp_method=1, no_s=True)
    assert list(only_s[0]) == ["prob_thre", "tp_thre"] + [f"s_{k}" for k in PHASE_KEYS]
    assert list(only_p[0]) == ["prob_thre", "tp_thre"] + [f"p_{k}" for k in PHASE_KEYS]
    for j in range(3):
        assert all(same_number(only_s[j][k], both[j][k]) for k in only_s[j])
        assert all(same_number(only_p[j][k], both[j][k]) for k in only_p[j])
    r1 = E.task0_residuals(p_truth, count[:, 0], peak[:, 0], start, method=1)[0]
    assert both[0]["p_mean"] == np.mean(r1) and len(r1) <= (~np.isnan(p_truth)).sum()
    with pytest.raises(ValueError):
        E.task0_metrics(p_truth, s_truth, count, peak, start, thr, no_p=True, no_s=True)
    with pytest.raises(ValueError):
        E.task0_metrics(p_truth, s_truth, count, peak, start, thr[:2])


def test_truth_is_the_first_onset_inside_the_target():
    onsets = np.full((4, 4), np.nan)
    onsets[0] = [100, 900, 400, np.nan]   # two P, one S
    onsets[1] = [250.5, np.nan, np.nan, np.nan]
    onsets[3] = [np.nan, np.nan, 50, 60]
    bank = SimpleNamespace(onsets=onsets)
    targets = {"trace": np.array([0, 0, 0, 1, 1, 2, 3, 3]),
               "start_sample": np.array([0, 100, 101, 250, 251, 0, 50, 0]),
               "end_sample": np.array([100, 500, 1000, 251, 300, 10, 51, 50])}
    p, s = E.task0_truth(bank, targets)
    #                  end excluded  start included  the FIRST P only            250 <= 250.5 < 251
    assert np.array_equal(p, [np.nan, 100, np.nan, 250.5, np.nan, np.nan, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(s, [np.nan, 400, 400, np.nan, np.nan, np.nan, 50, np.nan], equal_nan=True)
    assert p.dtype == s.dtype == np.float64
    p, s = E.task0_truth(bank, targets, p_truth=np.full(8, 60.0), s_truth=[np.nan] * 8)
    assert np.array_equal(p, [60, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan], equal_nan=True) and np.isnan(s).all()


def test_true_negative_rows_by_hand():
    p_truth = np.array([np.nan, np.nan, np.nan, 10.0, 20.0])
    s_truth = np.array([1.0, 2.0, 3.0, 4.0, 5.0])  # no target without an S onset
    count = np.zeros((5, 2, 2), np.int32)
    count[:, 0, 0] = [0, 2, 1, 3, 0]
    count[:, 0, 1] = [0, 0, 1, 0, 0]
    count[:, 1, 0] = 1
    rows = E.task0_tnr(p_truth, s_truth, count, [0.2, 0.6])
    assert list(rows[0]) == ["prob_thre", "p_TN", "p_FP", "p_true_negative_rate", "s_TN", "s_FP", "s_true_negative_rate"]
    assert (rows[0]["prob_thre"], rows[0]["p_TN"], rows[0]["p_FP"], rows[0]["p_true_negative_rate"]) == (0.2, 1, 2, 1 / 3)
    assert (rows[1]["p_TN"], rows[1]["p_FP"], rows[1]["p_true_negative_rate"]) == (2, 1, 2 / 3)
    assert (rows[0]["s_TN"], rows[0]["s_FP"]) == (0, 0) and np.isnan(rows[0]["s_true_negative_rate"])


def test_optimal_thresholds_by_hand():
    def table(p_f1, s_f1, tag):
        return [{"prob_thre": t, "tp_thre": 0.5, "p_TP": tag + 10 * i, "p_F1score": p, "s_TP": tag + 100 * i, "s_F1score": s}
                for i, (t, p, s) in enumerate(zip((0.1, 0.2, 0.3, 0.4), p_f1, s_f1))]

    dev = table([0.5, 0.8, 0.8, 0.1], [0.2, 0.3, 0.4, 0.9], 1)
    test = table([0.9, 0.1, 0.9, 0.9], [0.9, 0.9, 0.9, 0.1], 2)
    got = E.opt_prob_metrics(dev, test)
    assert list(got) == ["tp_thre", "p_opt_prob_thre", "s_opt_prob_thre", "test_p_TP", "test_p_F1score", "test_s_TP",
                         "test_s_F1score", "dev_p_TP", "dev_p_F1score", "dev_s_TP", "dev_s_F1score"]
    # P: the FIRST of the two best dev rows (0.2); S: the last row; the test rows are the dev optimum's, not test's own
    assert (got["p_opt_prob_thre"], got["s_opt_prob_thre"], got["tp_thre"]) == (0.2, 0.4, 0.5)
    assert (got["test_p_TP"], got["test_p_F1score"], got["dev_p_TP"], got["dev_p_F1score"]) == (12, 0.1, 11, 0.8)
    assert (got["test_s_TP"], got["test_s_F1score"], got["dev_s_TP"], got["dev_s_F1score"]) == (302, 0.1, 301, 0.9)
    # a NaN F1 (no picks at a threshold) counts as the largest, as np.argmax on the reference's table does
    dev[2]["p_F1score"] = np.nan
    assert E.opt_prob_metrics(dev, test)["p_opt_prob_thre"] == 0.3
    pd = pytest.importorskip("pandas")
    assert E.opt_prob_metrics(pd.DataFrame(dev), pd.DataFrame(test))["s_opt_prob_thre"] == 0.4


def test_threshold_grids():
    on, off, select = E._sweep_grid(np.arange(0.1, 1.0, 0.1))
    assert on.dtype == off.dtype == np.float32 and select is None and len(on) == 9
    assert np.array_equal(on, R.thresholds(R.GRID)[0]) and np.array_equal(off, R.thresholds(R.GRID)[1])
    assert np.array_equal(off * np.float32(2), on)
    on, off, select = E._sweep_grid(0.3)
    assert on.tolist() == [np.float32(0.3)] and select is None
    on, off, select = E._sweep_grid([[0.5, 0.3], [0.3, 0.7]])
    assert on.tolist() == [np.float32(0.3), np.float32(0.5), np.float32(0.7)]
    assert select[0].tolist() == [1, 0] and select[1].tolist() == [0, 2]
    count = np.arange(2 * 2 * 3).reshape(2, 2, 3).astype(np.int32) % 4
    peak = np.arange(2 * 2 * 3 * 4).reshape(2, 2, 3, 4).astype(np.int32)
    c, p, v = E._sweep_result(count, peak, None, select, 4)
    assert v is None and c.shape == (2, 2, 2) and p.shape == (2, 2, 2, 4)
    assert np.array_equal(c[:, 0], count[:, 0][:, [1, 0]]) and np.array_equal(p[:, 1], peak[:, 1][:, [0, 2]])
    with pytest.raises(RuntimeError, match="max_picks"):
        E._sweep_result(count, peak, None, None, 2)
    for bad in ([], np.zeros(33), [np.nan], np.zeros((3, 2, 2))):
        with pytest.raises(ValueError):
            E._sweep_grid(bad)


@pytest.mark.parametrize("seed", range(4))
def test_the_restatement_equals_the_oracle_on_random_traces(seed):
    rng = np.random.default_rng(seed)
    n = [3001, 6000, 257, 1][seed]
    x = np.clip(np.convolve(rng.random(n + 16) ** 4, np.ones(17) / 17, "valid") * 4, 0, 1).astype(np.float32)
    x[rng.integers(0, n, n // 200 + 1)] = 1.0  # ties among the maxima
    on, off = R.thresholds(R.GRID)
    total = 0
    for j in range(9):
        want = picks_from_trace(x, on[j], off[j])
        peaks, values = R.picks(x, on[j], off[j])
        assert peaks.tolist() == [w[2] for w in want] and values.tolist() == [np.float32(w[3]) for w in want]
        assert (np.diff(peaks) > 0).all()
        total += len(peaks)
    count, peak, value = R.sweep(x[None, None].repeat(2, 1), 0, 1, on, off, 4)
    assert np.array_equal(count[0, 0], count[0, 1]) and count.sum() == 2 * total
    for j in range(9):
        peaks, values = R.picks(x, on[j], off[j])
        k = min(4, len(peaks))
        assert peak[0, 0, j, :k].tolist() == peaks[:k].tolist() and (peak[0, 0, j, k:] == -1).all()
        assert value[0, 1, j, :k].tolist() == values[:k].tolist() and (value[0, 1, j, k:] == 0).all()
    assert seed == 3 or total > 0


def test_the_adversarial_rows_are_what_they_say():
    """Each row kind against its own threshold pair: the properties the GPU test leans on."""
    T = 3001
    on, off = (np.float32(v) for v in (0.3, 0.15))
    rng = np.random.default_rng(1)

    def row(kind, a=200, e=2700):
        x = np.zeros(T, np.float32)
        kind(rng, x, a, e, on, off)
        return x, R.picks(x[a:e], on, off)[0]

    assert len(row(R._quiet)[1]) == 0 and len(row(R._between_only)[1]) == 0
    x, pk = row(R._plateau_at_on)
    assert len(pk) == 0 and (x == on).sum() == 20
    x, pk = row(R._whole)
    assert len(pk) == 1 and (x[200:2700] > off).all()
    x, pk = row(R._cut_lo)
    assert len(pk) == 1 and x[199] == 1.0 and 0 <= pk[0] < 30
    x, pk = row(R._cut_hi)
    assert len(pk) == 1 and x[2700] == 1.0 and pk[0] >= 2470
    assert row(R._edge_peaks)[1].tolist() == [0, 2499]
    x, pk = row(R._two_bumps)
    assert len(pk) == 1 and 1535 <= pk[0] + 200 < 1540
    assert row(R._equal_maxima)[1].tolist() == [150]
    assert len(row(R._nan_in_run)[1]) == 2
    assert len(row(R._single_gap)[1]) > 10
    assert len(row(R._spikes)[1]) > 64
    for kind in R.ROW_KINDS:  # and every kind fits every border, the one-sample ones included
        for a, e in R.border_cases(T):
            row(kind, a, e)
    prob, lo, hi = R.adversarial_batch(T, 37, 0, 1, 2)
    assert prob.shape == (37, 3, T) and prob.dtype == np.float32 and np.isnan(prob).any()
    assert ((lo >= 0) & (hi <= T) & (hi > lo)).all() and len(set(zip(lo.tolist(), hi.tolist()))) == len(R.border_cases(T))
