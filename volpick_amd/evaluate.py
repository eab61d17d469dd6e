"""The reference's own window-level evaluation protocol on the MI355X path.

Mirrors ``evaluate()`` of volpick/model/eval_taks0.py:20-200 for pre-cut, already normalised
windows: forward pass, slice ``window_borders``, ``trigger_onset(prob, thr, thr / 2)`` and per
trigger ``max`` / ``argmax`` (``get_picks_from_prob``, eval_taks0.py:46-56).  The per-sample
Python loop of the reference (eval_taks0.py:96-142) runs as one kernel launch per phase
(``vp_pick_windows``).  Dataset handling, TP/FP/FN counting and CSV bookkeeping stay out of scope.

The pick-benchmark tasks 1-3 (volpick/model/eval_taks123.py) are here as well.  ``predict_windows`` is ``predict_step``
of the reference's Lightning modules (models.py:454-480, :881-906) on pre-cut windows, ``eval_tasks123`` the pass of
eval_taks123.py:137-160 over a :class:`~volpick_amd.generate.WaveformBank` -- windows placed by
:class:`~volpick_amd.generate.SteeredPlanner`, cut, normalised, predicted and reduced on the GPU with one host wait
(``vp_predict_begin`` / ``_bank`` / ``_end``) -- and ``task1_metrics`` / ``task23_metrics`` restate ``parse_task1`` /
``parse_task23`` (:231-415) in numpy.  The kernel returns the P and S maxima; ``score_p_or_s`` is their float32 quotient,
formed here on the host (numpy's division: correctly rounded, ``x / 0 = inf``, ``0 / 0 = NaN``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def evaluate_windows(model, X, window_borders=None, threshold=0.3, batch_size=1024, max_picks=64):
    """X: (N, 3, T) float32, normalised as the reference's generator does
    (``Normalize(demean_axis=-1, amp_norm_axis=-1, amp_norm_type=model.norm)``, eval_taks0.py:458-469).
    window_borders: (N, 2) int [start, end) local sample ranges, or None for whole windows.
    threshold: float, or [P_threshold, S_threshold].

    Returns ``[p_picks, p_scores, s_picks, s_scores]``: four lists with one ndarray per window
    (pick samples are local to the window border start, ascending), the first four entries of the
    reference's ``merged_predictions`` before the per-trace ``start_sample`` offset is added.
    """
    torch = __import__("torch")
    lib = _lib.load()
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    p_thr, s_thr = (threshold if isinstance(threshold, (list, tuple)) else (threshold, threshold))
    if model.name == "PhaseNet":
        rows = {"P": model.labels.index("P"), "S": model.labels.index("S")}
    else:  # EQTransformer returns (detection, P, S)
        rows = {"P": 1, "S": 2}
    lo = hi = None
    if window_borders is not None:
        wb = np.asarray(window_borders, dtype=np.int32).reshape(n, 2)
        lo, hi = np.ascontiguousarray(wb[:, 0]), np.ascontiguousarray(wb[:, 1])
    out = {ph: ([], []) for ph in rows}
    h = model._ensure_handle()
    for b0 in range(0, n, batch_size):
        xb = torch.from_numpy(X[b0 : b0 + batch_size]).to(model.device)
        y = model._forward_raw(xb)  # (B, 3, T) on the device
        B = y.shape[0]
        for ph, thr in (("P", p_thr), ("S", s_thr)):
            count = np.zeros(B, np.int32)
            peak = np.zeros((B, max_picks), np.int32)
            value = np.zeros((B, max_picks), np.float32)
            plo = lo[b0 : b0 + B].ctypes.data_as(C.c_void_p) if lo is not None else None
            phi = hi[b0 : b0 + B].ctypes.data_as(C.c_void_p) if hi is not None else None
            _lib.check(lib.vp_pick_windows(h, C.c_void_p(y.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, rows[ph], plo, phi,
                                           float(thr), float(thr) / 2.0, max_picks,
                                           count.ctypes.data_as(C.c_void_p), peak.ctypes.data_as(C.c_void_p),
                                           value.ctypes.data_as(C.c_void_p)), "vp_pick_windows")
            if (count > max_picks).any():
                raise RuntimeError(f"more than max_picks={max_picks} triggers in a window; raise max_picks")
            for i in range(B):
                k = count[i]
                order = np.argsort(peak[i, :k], kind="stable")
                out[ph][0].append(peak[i, :k][order].astype(np.int64))
                out[ph][1].append(value[i, :k][order])
    return [out["P"][0], out["P"][1], out["S"][0], out["S"][1]]


# ---- pick-benchmark tasks 1-3 ------------------------------------------------------------------------------------------
RECORD = np.dtype([("det", np.float32), ("p_max", np.float32), ("s_max", np.float32), ("p_arg", np.int32), ("s_arg", np.int32)])
assert RECORD.itemsize == C.sizeof(_lib.VpPredictRecord)


def _predict_rows(model):
    """(det_row, p_row, s_row, det_mode) of the model's (B, 3, T) output."""
    if model.name == "PhaseNet":
        return model.labels.index("N"), model.labels.index("P"), model.labels.index("S"), _lib.VP_DET_ONE_MINUS_NOISE
    return 0, 1, 2, _lib.VP_DET_ROW  # EQTransformer returns (detection, P, S)


def _scores(rec):
    """Records -> predict_step's tuple: (score_detection, score_p_or_s, p_sample, s_sample)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        p_or_s = rec["p_max"] / rec["s_max"]  # float32 / float32
    return rec["det"].copy(), p_or_s, rec["p_arg"].astype(np.int64), rec["s_arg"].astype(np.int64)


def _borders(window_borders, n):
    if window_borders is None:
        return None, None
    wb = np.asarray(window_borders, dtype=np.int32).reshape(n, 2)
    return np.ascontiguousarray(wb[:, 0]), np.ascontiguousarray(wb[:, 1])


def predict_windows(model, X, window_borders=None, batch_size=1024):
    """``predict_step`` of the reference on X: (N, 3, T) float32 windows, cut and normalised as its generator does.
    window_borders: (N, 2) int [start, end) local sample ranges, or None for whole windows.

    Returns ``(score_detection, score_p_or_s, p_sample, s_sample)``: float32, float32, int64, int64 arrays of N, the samples
    local to the border start.  PhaseNet: ``max(1 - noise)``; EQTransformer: the maximum of its detection trace."""
    torch = __import__("torch")
    lib = _lib.load()
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    lo, hi = _borders(window_borders, n)
    det_row, p_row, s_row, mode = _predict_rows(model)
    rec = np.zeros(n, RECORD)
    h = model._ensure_handle()
    for b0 in range(0, n, batch_size):
        y = model._forward_raw(torch.from_numpy(X[b0 : b0 + batch_size]).to(model.device))  # (B, 3, T) on the device
        B = y.shape[0]
        plo = lo[b0 : b0 + B].ctypes.data_as(C.c_void_p) if lo is not None else None
        phi = hi[b0 : b0 + B].ctypes.data_as(C.c_void_p) if hi is not None else None
        _lib.check(lib.vp_predict_windows(h, C.c_void_p(y.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, det_row, p_row, s_row, mode,
                                          plo, phi, rec[b0 : b0 + B].ctypes.data_as(C.c_void_p)), "vp_predict_windows")
    return _scores(rec)


def predict_bank(model, bank, rows, window_borders=None, batch_size=1024, predictions=False):
    """One prediction pass on the GPU (``vp_predict_begin`` ... ``vp_predict_end``): the plan ``rows`` are cut from ``bank``
    and normalised with ``model.norm``, predicted and reduced in batches of ``batch_size``; the host waits once, at the end.
    Returns ``predict_windows``' tuple; with ``predictions=True`` also the list of the batches' (B, 3, T) probabilities
    (CUDA tensors)."""
    from .generate import _norm, as_rows

    lib = _lib.load()
    rows = as_rows(rows)
    n = len(rows)
    lo, hi = _borders(window_borders, n)
    det_row, p_row, s_row, _ = _predict_rows(model)
    if model._device_index is None:
        model.cuda(bank.device)
    h = model._ensure_handle()
    preds = []
    if predictions:
        torch = __import__("torch")
        dev = torch.device("cuda", model._device_index)
    rec = np.zeros(n, RECORD)
    _lib.check(lib.vp_predict_begin(h), "vp_predict_begin")
    try:
        for b0 in range(0, n, batch_size):
            r = rows[b0 : b0 + batch_size]
            B = len(r)
            out = None
            if predictions:
                out = torch.empty((B, 3, model.in_samples), dtype=torch.float32, device=dev)
                torch.cuda.current_stream(dev).synchronize()  # whatever used this memory last on torch's stream is done
                preds.append(out)
            plo = lo[b0 : b0 + B].ctypes.data_as(C.c_void_p) if lo is not None else None
            phi = hi[b0 : b0 + B].ctypes.data_as(C.c_void_p) if hi is not None else None
            _lib.check(lib.vp_predict_bank(h, bank.handle, r.ctypes.data_as(C.c_void_p), plo, phi, B, _norm(model.norm), det_row,
                                           p_row, s_row, C.c_void_p(out.data_ptr()) if predictions else None), "vp_predict_bank")
    finally:
        nw = C.c_longlong()
        rc = lib.vp_predict_end(h, rec.ctypes.data_as(C.c_void_p), n, C.byref(nw))
    _lib.check(rc, "vp_predict_end")
    assert nw.value == n
    return _scores(rec) + ((preds,) if predictions else ())


def _columns(table):
    """A DataFrame or a dict of arrays -> {column: ndarray}."""
    return {k: np.asarray(table[k]) for k in table.keys()}


def eval_tasks123(model, bank, targets, batch_size=1024):
    """The prediction pass of the reference's ``eval_tasks123`` (eval_taks123.py:137-160) for one set of task targets:
    ``targets`` (a DataFrame or a dict of arrays) holds ``trace`` (the bank index), ``start_sample`` and ``end_sample``.
    Returns the targets -- a DataFrame copy for a DataFrame, else a dict -- with ``score_detection``, ``score_p_or_s``,
    ``p_sample_pred`` and ``s_sample_pred`` added, the samples counted from the trace start (``start_sample`` added).
    Target files, sets and directories are the caller's."""
    from .generate import SteeredPlanner

    rows, borders = SteeredPlanner(bank, model.in_samples).plan(targets)
    det, p_or_s, p_arg, s_arg = predict_bank(model, bank, rows, borders, batch_size)
    out = dict(targets) if isinstance(targets, dict) else targets.copy()
    start = np.asarray(targets["start_sample"])
    out["score_detection"] = det
    out["score_p_or_s"] = p_or_s
    out["p_sample_pred"] = p_arg + start
    out["s_sample_pred"] = s_arg + start
    return out


def _pr_curve(y, score):
    """Precision, recall (each one longer than the thresholds: the closing point (1, 0)) and the ascending distinct
    thresholds, a sample counted positive when ``score >= threshold`` -- sklearn's ``precision_recall_curve``."""
    y = np.asarray(y, bool)
    score = np.asarray(score, np.float64)
    if y.size == 0 or np.isnan(score).any():
        raise ValueError("precision-recall curve: no samples, or a NaN score")
    order = np.argsort(score, kind="stable")[::-1]
    score, y = score[order], y[order]
    last = np.r_[np.flatnonzero(np.diff(score)), y.size - 1]  # the last sample of every distinct score, descending
    tp = np.cumsum(y)[last].astype(np.float64)
    pred = (last + 1).astype(np.float64)
    prec = tp / pred
    rec = tp / tp[-1] if tp[-1] > 0 else np.ones_like(tp)
    return np.r_[prec[::-1], 1.0], np.r_[rec[::-1], 0.0], score[last][::-1]


def _f1_optimum(y, score):
    """(precision, recall, F1, threshold) where F1 = 2 p r / (p + r) is largest on the curve (the first such point)."""
    prec, rec, thr = _pr_curve(y, score)
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = 2 * prec * rec / (prec + rec)
    i = int(np.nanargmax(f1))
    return prec[i], rec[i], f1[i], thr[i]


def _roc_auc(y, score):
    """The probability that a positive outscores a negative, ties counting a half (rank form of Mann-Whitney's U)."""
    y = np.asarray(y, bool)
    score = np.asarray(score, np.float64)
    if np.isnan(score).any():
        raise ValueError("ROC AUC: a NaN score")
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("ROC AUC is not defined with one class only")
    uniq, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    upper = np.cumsum(cnt)
    rank = (upper - (cnt - 1) / 2.0)[inv]  # average 1-based rank
    return float((rank[y].sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg))


def _confusion(y, pred):
    y, pred = np.asarray(y, bool), np.asarray(pred, bool)
    return int((y & pred).sum()), int((~y & pred).sum()), int((y & ~pred).sum()), int((~y & ~pred).sum())  # tp fp fn tn


def _prf(y, pred):
    """Precision, recall and F1 = 2 tp / (2 tp + fp + fn) of the positive class; 0 where a denominator is."""
    tp, fp, fn, _ = _confusion(y, pred)
    div = lambda a, b: a / b if b else 0.0
    return div(tp, tp + fp), div(tp, tp + fn), div(2 * tp, 2 * tp + fp + fn)


def _mcc(y, pred):
    tp, fp, fn, tn = _confusion(y, pred)
    den = (tp + fp) * (tp + fn) * (tn + fp) * (tn + fn)
    return float(tp * tn - fp * fn) / float(np.sqrt(float(den))) if den else 0.0


def task1_metrics(dev, test):
    """``parse_task1`` (eval_taks123.py:231-278): ``dev`` / ``test`` hold ``trace_type`` ("earthquake" is the positive class)
    and ``score_detection``.  The detection threshold is the F1 optimum of the dev precision-recall curve; the test set is
    scored with ``score_detection > threshold``."""
    dev, test = _columns(dev), _columns(test)
    y_dev, y_test = dev["trace_type"] == "earthquake", test["trace_type"] == "earthquake"
    prec, rec, f1, thr = _f1_optimum(y_dev, dev["score_detection"])
    stats = {"dev_det_precision": prec, "dev_det_recall": rec, "dev_det_f1": f1,
             "dev_det_auc": _roc_auc(y_dev, dev["score_detection"]), "det_threshold": thr}
    prec, rec, f1 = _prf(y_test, test["score_detection"] > thr)
    stats.update({"test_det_precision": prec, "test_det_recall": rec, "test_det_f1": f1,
                  "test_det_auc": _roc_auc(y_test, test["score_detection"])})
    return stats


N_MCC_CANDIDATES = 50  # thresholds tried for the MCC optimum: evenly spaced ranks of the sorted dev scores
RESIDUAL_BOUND_S = 1   # the "modified" residual statistics keep |residual| < 1 s; "out" is the fraction beyond it


def task23_metrics(dev, test):
    """``parse_task23`` (eval_taks123.py:281-415): ``dev`` / ``test`` hold ``phase_label`` ("P" / "S"), ``phase_onset``,
    ``sampling_rate``, ``p_sample_pred`` and, optionally, ``s_sample_pred`` and ``score_p_or_s`` (missing: NaN).  Rows whose
    three predictions are all NaN are dropped; ``{}`` when that leaves no dev row.  Task 2 is skipped where every dev or every
    test score is NaN or infinite; else the scores are clipped to +-1e100, the phase threshold is the dev F1 optimum over the
    rows with a score, the MCC threshold the best of ``N_MCC_CANDIDATES`` ranks of all dev scores, and both are applied to
    the test set with ``>``.  Task 3: per set and phase the residual ``(sample_pred - phase_onset) / sampling_rate`` in
    seconds: mean, RMSE and MAE with NaN residuals left out (the reference's ``np.mean`` of a pandas Series hands over to
    ``Series.mean``, which skips them), the median NaN as soon as one residual is (its ``np.median`` does not hand over), the
    fraction beyond ``RESIDUAL_BOUND_S`` over all rows of the phase, and RMSE / MAE of the residuals inside the bound."""
    import warnings

    def prepared(table):
        t = _columns(table)
        n = len(t["phase_label"])
        for col in ("s_sample_pred", "score_p_or_s"):
            if col not in t:
                t[col] = np.full(n, np.nan)
        t = {k: (v.astype(np.float64) if k in ("p_sample_pred", "s_sample_pred", "score_p_or_s") else v) for k, v in t.items()}
        t["_nan"] = np.isnan(t["p_sample_pred"]) & np.isnan(t["s_sample_pred"]) & np.isnan(t["score_p_or_s"])
        return t

    def keep(t, mask):
        return {k: v[mask] for k, v in t.items()}

    dev, test = prepared(dev), prepared(test)
    if dev["_nan"].all():
        return {}
    dev, test = keep(dev, ~dev["_nan"]), keep(test, ~test["_nan"])
    stats = {}
    skip_task2 = any((np.isnan(t["score_p_or_s"]) | np.isinf(t["score_p_or_s"])).all() for t in (dev, test))
    for t in (dev, test):
        t["score_p_or_s"] = np.clip(t["score_p_or_s"], -1e100, 1e100)
        t["_is_p"] = t["phase_label"] == "P"
    dev_r, test_r = keep(dev, ~np.isnan(dev["score_p_or_s"])), keep(test, ~np.isnan(test["score_p_or_s"]))
    if len(dev_r["_is_p"]) > 0 and not skip_task2:
        prec, rec, f1, thr = _f1_optimum(dev_r["_is_p"], dev_r["score_p_or_s"])
        cand = np.sort(dev["score_p_or_s"])  # (NaN last: a NaN candidate predicts no P at all)
        cand = cand[np.linspace(0, len(cand) - 1, N_MCC_CANDIDATES, dtype=int)]
        with np.errstate(invalid="ignore"):
            mccs = [_mcc(dev["_is_p"], dev["score_p_or_s"] > c) for c in cand]
            best = int(np.argmax(mccs))
            stats.update({"dev_phase_precision": prec, "dev_phase_recall": rec, "dev_phase_f1": f1, "phase_threshold": thr,
                          "dev_phase_mcc": mccs[best], "phase_threshold_mcc": cand[best]})
            prec, rec, f1 = _prf(test_r["_is_p"], test_r["score_p_or_s"] > thr)
            stats.update({"test_phase_precision": prec, "test_phase_recall": rec, "test_phase_f1": f1,
                          "test_phase_mcc": _mcc(test["_is_p"], test["score_p_or_s"] > cand[best])})
    for t, name in ((dev, "dev"), (test, "test")):
        for phase in ("P", "S"):
            m = t["phase_label"] == phase
            if not m.any():
                continue
            diff = (t[f"{phase.lower()}_sample_pred"][m] - t["phase_onset"][m]) / t["sampling_rate"][m]
            inside = diff[(diff < RESIDUAL_BOUND_S) & (diff > -RESIDUAL_BOUND_S)]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # a mean of nothing is NaN, as in the reference
                stats[f"{name}_{phase}_mean_s"] = np.nanmean(diff)
                stats[f"{name}_{phase}_median_s"] = np.median(diff)  # (np.median does not hand over to pandas: NaN stays)
                stats[f"{name}_{phase}_rmse_s"] = np.sqrt(np.nanmean(diff**2))
                stats[f"{name}_{phase}_mae_s"] = np.nanmean(np.abs(diff))
                stats[f"{name}_{phase}_out_s"] = int(((diff > RESIDUAL_BOUND_S) | (diff < -RESIDUAL_BOUND_S)).sum()) / len(diff)
                stats[f"{name}_{phase}_modified_rmse_s"] = np.sqrt(np.mean(inside**2))
                stats[f"{name}_{phase}_modified_mae_s"] = np.mean(np.abs(inside))
    return stats
