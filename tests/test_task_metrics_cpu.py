"""CPU: evaluate.task1_metrics / task23_metrics -- parse_task1 / parse_task23 of the reference (volpick/model/eval_taks123.py:
231-415) in numpy.  Always: the definitions (pair counting, confusion-matrix formulas, a brute-force threshold search).
Where sklearn and pandas are importable: the same protocol written with sklearn.metrics."""
import numpy as np
import pytest

from volpick_amd import evaluate as E

RTOL = 1e-12


def task1_tables(seed, n=400, decimals=2):
    """Seeded detection scores with ties (rounded to `decimals`), earthquakes scoring higher on average."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        quake = rng.random(n) < 0.6
        score = np.clip(rng.normal(np.where(quake, 0.7, 0.4), 0.2), 0, 1).round(decimals).astype(np.float32)
        out.append({"trace_type": np.where(quake, "earthquake", "noise"), "score_detection": score})
    return out


def task23_tables(seed, n=300, decimals=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        is_p = rng.random(n) < 0.5
        score = np.exp(rng.normal(np.where(is_p, 1.0, -1.0), 1.0)).round(decimals).astype(np.float32)
        onset = rng.integers(500, 2500, n).astype(np.float64)
        p_pred = onset + np.where(is_p, rng.normal(0, 60, n), rng.normal(0, 300, n)).round()
        s_pred = onset + np.where(is_p, rng.normal(0, 300, n), rng.normal(0, 80, n)).round()
        out.append({"phase_label": np.where(is_p, "P", "S"), "phase_onset": onset, "sampling_rate": np.full(n, 100.0),
                    "score_p_or_s": score, "p_sample_pred": p_pred, "s_sample_pred": s_pred})
    return out


def confusion(y, pred):
    tp = sum(1 for a, b in zip(y, pred) if a and b)
    fp = sum(1 for a, b in zip(y, pred) if not a and b)
    fn = sum(1 for a, b in zip(y, pred) if a and not b)
    tn = sum(1 for a, b in zip(y, pred) if not a and not b)
    return tp, fp, fn, tn


def prf_by_formula(y, pred):
    tp, fp, fn, _ = confusion(y, pred)
    p = tp / (tp + fp) if tp + fp else 0.0
    r = tp / (tp + fn) if tp + fn else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def mcc_by_formula(y, pred):
    tp, fp, fn, tn = confusion(y, pred)
    den = (tp + fp) * (tp + fn) * (tn + fp) * (tn + fn)
    return (tp * tn - fp * fn) / den**0.5 if den else 0.0


def auc_by_pairs(y, score):
    pos, neg = score[y].astype(np.float64), score[~y].astype(np.float64)
    wins = (pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()
    return wins / (len(pos) * len(neg))


def best_f1_by_search(y, score):
    """Every distinct score as a threshold with >=, ascending; the first largest F1 = 2 p r / (p + r)."""
    best = None
    for thr in np.unique(score):
        p, r, _ = prf_by_formula(y, score >= thr)
        f1 = 2 * p * r / (p + r) if p + r else np.nan
        if not np.isnan(f1) and (best is None or f1 > best[2]):
            best = (p, r, f1, thr)
    return best


@pytest.mark.parametrize("seed", range(3))
def test_task1_by_the_definitions(seed):
    dev, test = task1_tables(seed)
    got = E.task1_metrics(dev, test)
    assert set(got) == {"dev_det_precision", "dev_det_recall", "dev_det_f1", "dev_det_auc", "det_threshold", "test_det_precision",
                        "test_det_recall", "test_det_f1", "test_det_auc"}
    y_dev, y_test = dev["trace_type"] == "earthquake", test["trace_type"] == "earthquake"
    p, r, f1, thr = best_f1_by_search(y_dev, dev["score_detection"])
    assert got["det_threshold"] == thr
    assert np.allclose([got["dev_det_precision"], got["dev_det_recall"], got["dev_det_f1"]], [p, r, f1], rtol=RTOL, atol=0)
    assert np.isclose(got["dev_det_auc"], auc_by_pairs(y_dev, dev["score_detection"]), rtol=RTOL, atol=0)
    assert np.isclose(got["test_det_auc"], auc_by_pairs(y_test, test["score_detection"]), rtol=RTOL, atol=0)
    want = prf_by_formula(y_test, test["score_detection"] > thr)  # strictly above, as the reference applies it
    assert np.allclose([got["test_det_precision"], got["test_det_recall"], got["test_det_f1"]], want, rtol=RTOL, atol=0)
    assert (test["score_detection"] == thr).any()  # the ties make > and >= differ on this set


def test_private_pieces_on_degenerate_inputs():
    y = np.array([True, True, False, False])
    assert E._roc_auc(y, np.array([1.0, 1.0, 1.0, 1.0])) == 0.5           # all tied
    assert E._roc_auc(y, np.array([0.9, 0.8, 0.8, 0.1])) == (2 + 1.5) / 4  # one tie across the classes
    assert E._roc_auc(y, np.array([np.inf, 3.0, 2.0, -np.inf])) == 1.0
    with pytest.raises(ValueError):
        E._roc_auc(np.array([True, True]), np.array([0.1, 0.2]))
    with pytest.raises(ValueError):
        E._roc_auc(y, np.array([0.1, np.nan, 0.3, 0.2]))
    assert E._prf(y, np.zeros(4, bool)) == (0.0, 0.0, 0.0)                 # nothing predicted
    assert E._mcc(y, np.ones(4, bool)) == 0.0 and E._mcc(np.ones(4, bool), y) == 0.0
    assert E._mcc(y, y) == 1.0 and E._mcc(y, ~y) == -1.0
    rng = np.random.default_rng(1)
    for _ in range(20):
        a, b = rng.random(50) < 0.4, rng.random(50) < 0.5
        assert np.isclose(E._mcc(a, b), mcc_by_formula(a, b), rtol=RTOL, atol=0)
        assert np.allclose(E._prf(a, b), prf_by_formula(a, b), rtol=RTOL, atol=0)


@pytest.mark.parametrize("seed", range(3))
def test_task23_by_the_definitions(seed):
    dev, test = task23_tables(seed)
    got = E.task23_metrics(dev, test)
    y_dev, y_test = dev["phase_label"] == "P", test["phase_label"] == "P"
    p, r, f1, thr = best_f1_by_search(y_dev, dev["score_p_or_s"])
    assert got["phase_threshold"] == thr
    assert np.allclose([got["dev_phase_precision"], got["dev_phase_recall"], got["dev_phase_f1"]], [p, r, f1], rtol=RTOL, atol=0)
    want = prf_by_formula(y_test, test["score_p_or_s"] > thr)
    assert np.allclose([got["test_phase_precision"], got["test_phase_recall"], got["test_phase_f1"]], want, rtol=RTOL, atol=0)
    cand = np.sort(dev["score_p_or_s"])[np.linspace(0, len(y_dev) - 1, 50, dtype=int)]  # 50 ranks of the sorted dev scores
    mccs = [mcc_by_formula(y_dev, dev["score_p_or_s"] > c) for c in cand]
    assert got["phase_threshold_mcc"] == cand[int(np.argmax(mccs))]
    assert np.isclose(got["dev_phase_mcc"], max(mccs), rtol=RTOL, atol=0)
    assert np.isclose(got["test_phase_mcc"], mcc_by_formula(y_test, test["score_p_or_s"] > got["phase_threshold_mcc"]), rtol=RTOL, atol=0)
    for t, name in ((dev, "dev"), (test, "test")):
        for ph in "PS":
            m = t["phase_label"] == ph
            d = (t[f"{ph.lower()}_sample_pred"][m] - t["phase_onset"][m]) / 100.0
            inside = d[np.abs(d) < 1]
            want = {"mean_s": d.mean(), "median_s": np.median(d), "rmse_s": np.sqrt((d**2).mean()), "mae_s": np.abs(d).mean(),
                    "out_s": (np.abs(d) > 1).sum() / len(d), "modified_rmse_s": np.sqrt((inside**2).mean()),
                    "modified_mae_s": np.abs(inside).mean()}
            for k, v in want.items():
                assert np.isclose(got[f"{name}_{ph}_{k}"], v, rtol=RTOL, atol=0), (name, ph, k)
            assert 0 < want["out_s"] < 1  # some residuals beyond 1 s, some within
    assert len(got) == 10 + 2 * 2 * 7


def special_tables():
    """Named edge cases: (dev, test) pairs."""
    cases = {}
    dev, test = task23_tables(7)
    dev["score_p_or_s"] = np.full(300, np.inf, np.float32)  # a model without S: every quotient x / 0
    cases["all_inf_dev"] = (dev, test)
    dev, test = task23_tables(8)
    test["score_p_or_s"] = np.where(np.arange(300) % 2 == 0, np.inf, np.nan).astype(np.float32)
    cases["inf_or_nan_test"] = (dev, test)
    dev, test = task23_tables(9)
    for t in (dev, test):  # rows 0-9 all NaN (dropped), 10-19 a NaN score only, 20-29 a NaN P sample only, some inf
        for k in ("score_p_or_s", "p_sample_pred", "s_sample_pred"):
            t[k] = t[k].astype(np.float64)
            t[k][:10] = np.nan
        t["score_p_or_s"][10:20] = np.nan
        t["p_sample_pred"][20:30] = np.nan
        t["score_p_or_s"][30:40] = np.inf
    cases["nan_rows"] = (dev, test)
    dev, test = task23_tables(10)
    for t in (dev, test):
        t["phase_label"] = np.full(300, "P")  # no S rows at all
    cases["no_s_rows"] = (dev, test)
    dev, test = task23_tables(11)
    for t in (dev, test):
        del t["s_sample_pred"], t["score_p_or_s"]  # a P-only model's files
    cases["p_only_columns"] = (dev, test)
    return cases


def test_task23_special_cases_without_sklearn():
    c = special_tables()
    for name in ("all_inf_dev", "inf_or_nan_test", "p_only_columns"):
        got = E.task23_metrics(*c[name])  # skip_task2: the residuals alone
        assert not any("phase" in k for k in got), name
        assert "dev_P_mean_s" in got and "test_P_rmse_s" in got
    got = E.task23_metrics(*c["no_s_rows"])
    assert not any("_S_" in k for k in got) and "dev_P_mae_s" in got
    assert got["dev_phase_mcc"] == 0.0 and got["dev_phase_recall"] == 1.0  # one class: MCC 0, everything is a P
    dev, test = c["nan_rows"]
    got = E.task23_metrics(dev, test)
    assert got["phase_threshold"] < 1e100
    for t, name in ((dev, "dev"), (test, "test")):
        # rows 20-29 have no P sample: the P rows among them leave the P median NaN (np.median keeps a NaN) while mean, RMSE
        # and MAE are those of the other P rows (rows 0-9 are dropped); every row counts in the out-fraction's denominator
        is_p = t["phase_label"][10:] == "P"
        assert is_p[10:20].any()
        d = ((t["p_sample_pred"][10:] - t["phase_onset"][10:]) / 100.0)[is_p]
        ok = d[~np.isnan(d)]
        assert np.isnan(got[f"{name}_P_median_s"]) and len(ok) < len(d)
        assert np.isclose(got[f"{name}_P_mean_s"], ok.mean(), rtol=RTOL, atol=0)
        assert np.isclose(got[f"{name}_P_rmse_s"], np.sqrt((ok**2).mean()), rtol=RTOL, atol=0)
        assert np.isclose(got[f"{name}_P_mae_s"], np.abs(ok).mean(), rtol=RTOL, atol=0)
        assert got[f"{name}_P_out_s"] == (np.abs(ok) > 1).sum() / len(d)
        assert np.isfinite([got[f"{name}_S_{k}"] for k in ("mean_s", "median_s", "rmse_s", "mae_s")]).all()  # every S sample is there
    dev, test = task23_tables(12)
    for k in ("score_p_or_s", "p_sample_pred", "s_sample_pred"):
        dev[k] = np.full(300, np.nan)
    assert E.task23_metrics(dev, test) == {}


# ------------------------------------------------------------------------------------------------- against sklearn.metrics
def sklearn_task1(dev, test):
    M = pytest.importorskip("sklearn.metrics")
    y_dev, y_test = dev["trace_type"] == "earthquake", test["trace_type"] == "earthquake"
    p, r, t = M.precision_recall_curve(y_dev, dev["score_detection"])
    with np.errstate(invalid="ignore"):
        f = 2 * p * r / (p + r)
    i = np.nanargmax(f)
    tp, tr, tf, _ = M.precision_recall_fscore_support(y_test, test["score_detection"] > t[i], average="binary")
    return {"dev_det_precision": p[i], "dev_det_recall": r[i], "dev_det_f1": f[i], "det_threshold": t[i],
            "dev_det_auc": M.roc_auc_score(y_dev, dev["score_detection"]), "test_det_precision": tp, "test_det_recall": tr,
            "test_det_f1": tf, "test_det_auc": M.roc_auc_score(y_test, test["score_detection"])}


def sklearn_task23(dev, test):
    """The protocol on pandas frames with sklearn's curve, scores and MCC."""
    M = pytest.importorskip("sklearn.metrics")
    pd = pytest.importorskip("pandas")
    frames = []
    for t in (dev, test):
        f = pd.DataFrame({k: v for k, v in t.items()})
        for col in ("s_sample_pred", "score_p_or_s"):
            if col not in f:
                f[col] = np.nan
        f["is_p"] = f["phase_label"] == "P"
        frames.append(f)
    all_nan = [f[["p_sample_pred", "s_sample_pred", "score_p_or_s"]].isna().all(axis=1) for f in frames]
    if all_nan[0].all():
        return {}
    dev, test = (f[~m].copy() for f, m in zip(frames, all_nan))
    skip = any((~np.isfinite(f["score_p_or_s"].to_numpy(np.float64))).all() for f in (dev, test))
    for f in (dev, test):
        f["score_p_or_s"] = np.clip(f["score_p_or_s"].to_numpy(np.float64), -1e100, 1e100)
    dev_r, test_r = dev[dev["score_p_or_s"].notna()], test[test["score_p_or_s"].notna()]
    out = {}
    if len(dev_r) and not skip:
        p, r, t = M.precision_recall_curve(dev_r["is_p"], dev_r["score_p_or_s"])
        with np.errstate(invalid="ignore"):
            f1 = 2 * p * r / (p + r)
        i = np.nanargmax(f1)
        cand = np.sort(dev["score_p_or_s"].to_numpy())
        cand = cand[np.linspace(0, len(cand) - 1, 50, dtype=int)]
        mccs = [M.matthews_corrcoef(dev["is_p"], dev["score_p_or_s"] > c) for c in cand]
        k = int(np.argmax(mccs))
        tp, tr, tf, _ = M.precision_recall_fscore_support(test_r["is_p"], test_r["score_p_or_s"] > t[i], average="binary")
        out.update({"dev_phase_precision": p[i], "dev_phase_recall": r[i], "dev_phase_f1": f1[i], "phase_threshold": t[i],
                    "dev_phase_mcc": mccs[k], "phase_threshold_mcc": cand[k], "test_phase_precision": tp, "test_phase_recall": tr,
                    "test_phase_f1": tf, "test_phase_mcc": M.matthews_corrcoef(test["is_p"], test["score_p_or_s"] > cand[k])})
    for f, name in ((dev, "dev"), (test, "test")):
        for ph in "PS":
            g = f[f["phase_label"] == ph]
            if len(g) == 0:
                continue
            # numpy's functions on a Series, as the reference calls them: np.mean hands over to Series.mean, which skips NaN;
            # np.median does not hand over and is NaN as soon as one residual is
            d = (g[f"{ph.lower()}_sample_pred"] - g["phase_onset"]) / g["sampling_rate"]
            inside = d[(d < 1) & (d > -1)]
            out.update({f"{name}_{ph}_mean_s": np.mean(d), f"{name}_{ph}_median_s": np.median(d),
                        f"{name}_{ph}_rmse_s": np.sqrt(np.mean(d**2)), f"{name}_{ph}_mae_s": np.mean(np.abs(d)),
                        f"{name}_{ph}_out_s": len(d[(d > 1) | (d < -1)]) / len(d),
                        f"{name}_{ph}_modified_rmse_s": np.sqrt(np.mean(inside**2)), f"{name}_{ph}_modified_mae_s": np.mean(np.abs(inside))})
    return out


THRESHOLDS = ("det_threshold", "phase_threshold", "phase_threshold_mcc")


def same_metrics(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        if k in THRESHOLDS or k.endswith("_out_s"):
            assert got[k] == v, k  # thresholds and counts: exact
        else:
            assert np.isclose(got[k], v, rtol=RTOL, atol=0, equal_nan=True), (k, got[k], v)


@pytest.mark.parametrize("seed", range(4))
def test_task1_equals_sklearn(seed):
    dev, test = task1_tables(seed, decimals=2 if seed % 2 else 6)
    same_metrics(E.task1_metrics(dev, test), sklearn_task1(dev, test))


@pytest.mark.parametrize("seed", range(4))
def test_task23_equals_sklearn(seed):
    dev, test = task23_tables(seed, decimals=1 if seed % 2 else 5)
    same_metrics(E.task23_metrics(dev, test), sklearn_task23(dev, test))


@pytest.mark.parametrize("name", ["all_inf_dev", "inf_or_nan_test", "nan_rows", "no_s_rows", "p_only_columns"])
def test_task23_special_cases_equal_sklearn(name):
    dev, test = special_tables()[name]
    want = sklearn_task23(dev, test)
    got = E.task23_metrics(dev, test)
    same_metrics(got, want)
    assert ("phase_threshold" in got) == (name in ("nan_rows", "no_s_rows"))


def test_dataframes_are_taken_as_dicts_are():
    pd = pytest.importorskip("pandas")
    dev, test = task1_tables(1)
    assert E.task1_metrics(pd.DataFrame(dev), pd.DataFrame(test)) == E.task1_metrics(dev, test)
    dev, test = task23_tables(1)
    a, b = E.task23_metrics(pd.DataFrame(dev), pd.DataFrame(test)), E.task23_metrics(dev, test)
    assert a.keys() == b.keys() and all(a[k] == b[k] for k in a)
