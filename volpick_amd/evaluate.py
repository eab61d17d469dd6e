"""The reference's own window-level evaluation protocol on the MI355X path.

Mirrors ``evaluate()`` of volpick/model/eval_taks0.py:20-200 for pre-cut, already normalised
windows: forward pass, slice ``window_borders``, ``trigger_onset(prob, thr, thr / 2)`` and per
trigger ``max`` / ``argmax`` (``get_picks_from_prob``, eval_taks0.py:46-56).  The per-sample
Python loop of the reference (eval_taks0.py:96-142) runs as one kernel launch per phase
(``vp_pick_windows``).

Task 0 itself (``eval_task0``, eval_taks0.py:370-825) runs from a :class:`~volpick_amd.generate.WaveformBank`: ``sweep_bank``
makes one forward pass per window and takes the picks of every threshold from it in one launch per batch (``vp_sweep_begin``
/ ``_bank`` / ``_end``; ``sweep_windows`` on pre-cut windows), and ``task0_truth``, ``task0_counts``, ``task0_residuals``,
``task0_metrics``, ``task0_tnr`` and ``opt_prob_metrics`` restate the reference's ground truth, TP/FP/FN counting, residual
statistics and tables in numpy.  Dataset handling and CSV bookkeeping stay out of scope.

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


def _predict_rows(model):
    """(det_row, p_row, s_row, det_mode) of the model's (B, 3, T) output."""
    if model.name == "PhaseNet":
        return model.labels.index("N"), model.labels.index("P"), model.labels.index("S"), _lib.VP_DET_ONE_MINUS_NOISE
    return 0, 1, 2, _lib.VP_DET_ROW  # EQTransformer returns (detection, P, S)


def _sweep_rows(model):
    return _predict_rows(model)[1:3]


def _borders(window_borders, n):
    if window_borders is None:
        return None, None
    wb = np.asarray(window_borders, dtype=np.int32).reshape(n, 2)
    return np.ascontiguousarray(wb[:, 0]), np.ascontiguousarray(wb[:, 1])


def _border_ptrs(lo, hi, b0, B):
    """Pointers to the borders of the windows [b0, b0 + B) for a C call; None each without borders."""
    return (None, None) if lo is None else (_lib.ptr(lo[b0 : b0 + B]), _lib.ptr(hi[b0 : b0 + B]))


def _forward_batches(model, X, window_borders, batch_size):
    """X: (N, 3, T) windows through the model in batches of ``batch_size``.  Yields ``(b0, B, y, lo, hi)`` per batch: its
    first window and size, its (B, 3, T) probabilities on the device, and the pointers to its borders (None without)."""
    torch = __import__("torch")
    lo, hi = _borders(window_borders, len(X))
    for b0 in range(0, len(X), batch_size):
        y = model._forward_raw(torch.from_numpy(X[b0 : b0 + batch_size]).to(model.device))
        B = y.shape[0]
        yield (b0, B, y) + _border_ptrs(lo, hi, b0, B)


def prediction_tensor(model, B):
    """A fresh (B, 3, T) float32 tensor on the model's device for a pass to write a batch's probabilities to.  The pass
    writes on the handle's stream, so whatever used this memory last on torch's stream is waited for here."""
    torch = __import__("torch")
    dev = torch.device("cuda", model._device_index)
    out = torch.empty((B, 3, model.in_samples), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    return out


def _bank_pass(model, bank, rows, window_borders, batch_size, predictions, name, begin, batch, end):
    """One pass over a bank on the GPU, its three C calls (``name``_begin / _bank / _end) supplied by the caller, each
    returning its code: ``begin(h)``; per ``batch_size`` of the plan ``rows`` (``as_rows``' array)
    ``batch(h, rows, lo, hi, B, out)`` -- pointers, ``lo`` / ``hi`` None without borders, ``out`` a fresh prediction tensor
    with ``predictions`` and else None; and in any case ``end(h, n, n_windows)``.  Returns the prediction tensors."""
    n = len(rows)
    lo, hi = _borders(window_borders, n)
    if model._device_index is None:
        model.cuda(bank.device)
    h = model._ensure_handle()
    preds = []
    _lib.check(begin(h), name + "_begin")
    try:
        for b0 in range(0, n, batch_size):
            r = rows[b0 : b0 + batch_size]
            B = len(r)
            if predictions:
                preds.append(prediction_tensor(model, B))
            out = C.c_void_p(preds[-1].data_ptr()) if predictions else None
            _lib.check(batch(h, _lib.ptr(r), *_border_ptrs(lo, hi, b0, B), B, out), name + "_bank")
    finally:
        nw = C.c_longlong()
        rc = end(h, n, C.byref(nw))
    _lib.check(rc, name + "_end")
    assert nw.value == n
    return preds


def evaluate_windows(model, X, window_borders=None, threshold=0.3, batch_size=1024, max_picks=64):
    """X: (N, 3, T) float32, normalised as the reference's generator does
    (``Normalize(demean_axis=-1, amp_norm_axis=-1, amp_norm_type=model.norm)``, eval_taks0.py:458-469).
    window_borders: (N, 2) int [start, end) local sample ranges, or None for whole windows.
    threshold: float, or [P_threshold, S_threshold].

    Returns ``[p_picks, p_scores, s_picks, s_scores]``: four lists with one ndarray per window
    (pick samples are local to the window border start, ascending), the first four entries of the
    reference's ``merged_predictions`` before the per-trace ``start_sample`` offset is added.
    """
    lib = _lib.load()
    X = np.ascontiguousarray(X, dtype=np.float32)
    thresholds = threshold if isinstance(threshold, (list, tuple)) else (threshold, threshold)
    out = ([], []), ([], [])  # per phase: picks, scores
    h = model._ensure_handle()
    for _, B, y, lo, hi in _forward_batches(model, X, window_borders, batch_size):
        for (picks, scores), row, thr in zip(out, _sweep_rows(model), thresholds):
            count = np.zeros(B, np.int32)
            peak = np.zeros((B, max_picks), np.int32)
            value = np.zeros((B, max_picks), np.float32)
            _lib.check(lib.vp_pick_windows(h, C.c_void_p(y.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, row, lo, hi, float(thr),
                                           float(thr) / 2.0, max_picks, _lib.ptr(count), _lib.ptr(peak), _lib.ptr(value)),
                       "vp_pick_windows")
            if (count > max_picks).any():
                raise RuntimeError(f"more than max_picks={max_picks} triggers in a window; raise max_picks")
            for i in range(B):
                k = count[i]
                order = np.argsort(peak[i, :k], kind="stable")
                picks.append(peak[i, :k][order].astype(np.int64))
                scores.append(value[i, :k][order])
    return [out[0][0], out[0][1], out[1][0], out[1][1]]


# ---- pick-benchmark tasks 1-3 ------------------------------------------------------------------------------------------
RECORD = np.dtype([("det", np.float32), ("p_max", np.float32), ("s_max", np.float32), ("p_arg", np.int32), ("s_arg", np.int32)])
assert RECORD.itemsize == C.sizeof(_lib.VpPredictRecord)


def _scores(rec):
    """Records -> predict_step's tuple: (score_detection, score_p_or_s, p_sample, s_sample)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        p_or_s = rec["p_max"] / rec["s_max"]  # float32 / float32
    return rec["det"].copy(), p_or_s, rec["p_arg"].astype(np.int64), rec["s_arg"].astype(np.int64)


def predict_windows(model, X, window_borders=None, batch_size=1024):
    """``predict_step`` of the reference on X: (N, 3, T) float32 windows, cut and normalised as its generator does.
    window_borders: (N, 2) int [start, end) local sample ranges, or None for whole windows.

    Returns ``(score_detection, score_p_or_s, p_sample, s_sample)``: float32, float32, int64, int64 arrays of N, the samples
    local to the border start.  PhaseNet: ``max(1 - noise)``; EQTransformer: the maximum of its detection trace."""
    lib = _lib.load()
    X = np.ascontiguousarray(X, dtype=np.float32)
    rec = np.zeros(len(X), RECORD)
    h = model._ensure_handle()
    for b0, B, y, lo, hi in _forward_batches(model, X, window_borders, batch_size):
        _lib.check(lib.vp_predict_windows(h, C.c_void_p(y.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, *_predict_rows(model), lo, hi,
                                          _lib.ptr(rec[b0 : b0 + B])), "vp_predict_windows")
    return _scores(rec)


def predict_bank(model, bank, rows, window_borders=None, batch_size=1024, predictions=False):
    """One prediction pass on the GPU (``vp_predict_begin`` ... ``vp_predict_end``): the plan ``rows`` are cut from ``bank``
    and normalised with ``model.norm``, predicted and reduced in batches of ``batch_size``; the host waits once, at the end.
    Returns ``predict_windows``' tuple; with ``predictions=True`` also the list of the batches' (B, 3, T) probabilities
    (CUDA tensors)."""
    from .generate import _norm, as_rows

    lib = _lib.load()
    rows = as_rows(rows)
    norm, rows3 = _norm(model.norm), _predict_rows(model)[:3]
    rec = np.zeros(len(rows), RECORD)
    preds = _bank_pass(model, bank, rows, window_borders, batch_size, predictions, "vp_predict", lib.vp_predict_begin,
                       lambda h, r, lo, hi, B, out: lib.vp_predict_bank(h, bank.handle, r, lo, hi, B, norm, *rows3, out),
                       lambda h, n, nw: lib.vp_predict_end(h, _lib.ptr(rec), n, nw))
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


# ---- pick-benchmark task 0 ---------------------------------------------------------------------------------------------
# The reference compares float32 probabilities with ``prob_thre`` inside ObsPy's trigger_onset.  With a Python float that is
# a float32 comparison under every NumPy; with the ``np.float64`` elements of ``np.arange(0.1, 1.0, 0.1)`` it is float32
# under NumPy 1's value-based casting and float64 under NumPy 2, and the reference pins no NumPy version.  The sweep rounds
# every threshold to float32 and compares in float32, which is ``vp_pick_windows``' and ``evaluate_windows``' contract.
SWEEP_COMPARE_DTYPE = np.float32
SWEEP_OFF_FRACTION = 2  # thr_off = thr_on / 2 (eval_taks0.py:46-56)
SWEEP_MAX_THRESHOLDS = 32
SWEEP_MAX_PICKS = 64
TASK0_SAMPLING_RATE = 100  # the reference hard-codes 100 Hz in its counts and residuals (eval_taks0.py:552, :573)


def _sweep_grid(thresholds):
    """``thresholds``: a number, NT numbers, or ``[P_thresholds, S_thresholds]`` (two rows of NT).  Returns the float32 on
    and off thresholds the kernel sweeps and, per phase, which of them are that phase's NT columns (None: all, in order)."""
    thr = np.asarray(thresholds, np.float64)
    if thr.ndim == 0:
        thr = thr[None]
    if thr.ndim == 2 and thr.shape[0] == 2:
        grid = np.unique(thr.astype(SWEEP_COMPARE_DTYPE))
        select = [np.searchsorted(grid, thr[ph].astype(SWEEP_COMPARE_DTYPE)) for ph in (0, 1)]
    elif thr.ndim == 1 and thr.size:
        grid, select = thr.astype(SWEEP_COMPARE_DTYPE), None
    else:
        raise ValueError("thresholds: a number, NT numbers or [P_thresholds, S_thresholds]")
    if grid.size > SWEEP_MAX_THRESHOLDS:
        raise ValueError(f"{grid.size} distinct thresholds; one sweep takes {SWEEP_MAX_THRESHOLDS}")
    if not np.isfinite(grid).all():
        raise ValueError("thresholds must be finite")
    on = np.ascontiguousarray(grid)
    return on, np.ascontiguousarray(on / SWEEP_COMPARE_DTYPE(SWEEP_OFF_FRACTION)), select


def _sweep_result(count, peak, value, select, max_picks):
    if select is not None:
        pick = lambda a: np.stack([a[:, ph][:, select[ph]] for ph in (0, 1)], axis=1)
        count, peak, value = pick(count), pick(peak), (None if value is None else pick(value))
    if (count > max_picks).any():
        raise RuntimeError(f"more than max_picks={max_picks} triggers in a window; raise max_picks")
    return count, peak, value


def _sweep_arrays(n, NT, K, scores):
    """The results of a sweep over n windows, as empty as the kernel leaves a window without picks."""
    return np.zeros((n, 2, NT), np.int32), np.full((n, 2, NT, K), -1, np.int32), (np.zeros((n, 2, NT, K), np.float32) if scores else None)


def sweep_windows(model, X, window_borders=None, thresholds=np.arange(0.1, 1.0, 0.1), batch_size=1024, max_picks=8,
                  scores=False):
    """The picks of ``evaluate_windows`` at every threshold of ``thresholds`` from ONE forward pass per window
    (``vp_sweep_windows``).  X and window_borders as for ``evaluate_windows``; ``thresholds``: NT numbers, or
    ``[P_thresholds, S_thresholds]`` as the reference's ``evaluate`` takes ``[p, s]``; ``thr_off = thr / 2``.

    Returns ``(count, peak, value)``: count (n, 2, NT) int32, phase 0 = P and 1 = S; peak (n, 2, NT, max_picks) int32, the
    pick samples local to the border start, ascending, -1 behind the count; value the float32 maxima (0 behind the count)
    with ``scores=True``, else None.  ``RuntimeError`` when a window has more than ``max_picks`` triggers."""
    lib = _lib.load()
    ptr = _lib.ptr
    X = np.ascontiguousarray(X, dtype=np.float32)
    on, off, select = _sweep_grid(thresholds)
    NT, K = len(on), int(max_picks)
    count, peak, value = _sweep_arrays(len(X), NT, K, scores)
    h = model._ensure_handle()
    for b0, B, y, lo, hi in _forward_batches(model, X, window_borders, batch_size):
        _lib.check(lib.vp_sweep_windows(h, C.c_void_p(y.data_ptr()), _lib.VP_MEM_DEVICE, B, 3, *_sweep_rows(model), lo, hi,
                                        ptr(on), ptr(off), NT, K, ptr(count[b0 : b0 + B]), ptr(peak[b0 : b0 + B]),
                                        ptr(None if value is None else value[b0 : b0 + B])), "vp_sweep_windows")
    return _sweep_result(count, peak, value, select, K)


def sweep_bank(model, bank, rows, window_borders=None, thresholds=np.arange(0.1, 1.0, 0.1), batch_size=1024, max_picks=8,
               scores=False, predictions=False):
    """One sweep pass on the GPU (``vp_sweep_begin`` ... ``vp_sweep_end``): the plan ``rows`` are cut from ``bank`` and
    normalised with ``model.norm``, predicted once and swept at every threshold in batches of ``batch_size``; the host waits
    once, at the end.  Returns ``sweep_windows``' tuple; with ``predictions=True`` also the list of the batches' (B, 3, T)
    probabilities (CUDA tensors)."""
    from .generate import _norm, as_rows

    lib = _lib.load()
    ptr = _lib.ptr
    rows = as_rows(rows)
    on, off, select = _sweep_grid(thresholds)
    NT, K = len(on), int(max_picks)
    norm, rows2 = _norm(model.norm), _sweep_rows(model)
    count, peak, value = _sweep_arrays(len(rows), NT, K, scores)
    preds = _bank_pass(model, bank, rows, window_borders, batch_size, predictions, "vp_sweep",
                       lambda h: lib.vp_sweep_begin(h, ptr(on), ptr(off), NT, K, int(scores)),
                       lambda h, r, lo, hi, B, out: lib.vp_sweep_bank(h, bank.handle, r, lo, hi, B, norm, *rows2, out),
                       lambda h, n, nw: lib.vp_sweep_end(h, ptr(count), ptr(peak), ptr(value), n, nw))
    return _sweep_result(count, peak, value, select, K) + ((preds,) if predictions else ())


def task0_truth(bank, targets, p_truth=None, s_truth=None):
    """``get_ground_truth`` (eval_taks0.py:203-239): per target the first P and the first S onset of its trace (``bank.onsets``;
    ``p_truth`` / ``s_truth``, one value per target, take their place when given), in trace samples; NaN where the trace
    has none or it lies outside the target's ``[start_sample, end_sample)``.  Returns ``(p, s)``, float64 arrays."""
    trace = np.asarray(targets["trace"], np.int64)
    start, end = np.asarray(targets["start_sample"]), np.asarray(targets["end_sample"])
    out = []
    for col, given in ((0, p_truth), (2, s_truth)):
        t = np.asarray(bank.onsets, np.float64).reshape(-1, 4)[trace, col] if given is None else np.array(given, np.float64)
        with np.errstate(invalid="ignore"):
            inside = (t >= start) & (t < end)
        out.append(np.where(inside, t, np.nan))
    return out[0], out[1]


def _picks(count, peak, start_sample):
    """(n, NT) counts and (n, NT, K) local peaks of one phase -> the picks in trace samples and which slots hold one."""
    count, peak = np.asarray(count), np.asarray(peak)
    held = np.arange(peak.shape[-1]) < count[..., None]
    return peak.astype(np.float64) + np.asarray(start_sample, np.float64)[:, None, None], held


def task0_counts(truth, count, peak, start_sample, tp_thre=0.5, sampling_rate=TASK0_SAMPLING_RATE, method=0):
    """``count_TP_FP_FN`` (eval_taks0.py:242-311) for one phase at every threshold: ``truth`` (n,) the onset per target or
    NaN (``task0_truth``), ``count`` (n, NT) and ``peak`` (n, NT, K) that phase's part of a sweep; the picks are
    ``peak + start_sample``.  A target without picks is a false negative if it has an onset.  With picks and no onset,
    method 0 counts every pick as a false positive and method 1 one per target.  With both, the target is a true positive
    when a pick lies within ``tp_thre`` seconds of the onset (``<=``); else it is a false negative (method 0) or a false
    positive (method 1); method 0 also counts each pick beyond ``tp_thre`` as a false positive.
    Returns ``(TP, FP, FN, tps, fps, fns)``: float64, the sums of shape (NT,) and the per-target arrays of shape (n, NT)."""
    if method not in (0, 1):
        raise ValueError("method must be 0 or 1")
    truth = np.asarray(truth, np.float64)
    picks, held = _picks(count, peak, start_sample)
    has_truth = ~np.isnan(truth)[:, None]
    has_picks = held.any(-1)
    with np.errstate(invalid="ignore"):
        near = held & (np.abs((picks - truth[:, None, None]) / sampling_rate) <= tp_thre)
    hit = near.any(-1)
    tps = (has_picks & has_truth & hit).astype(np.float64)
    if method == 0:
        fns = (has_truth & ~(has_picks & hit)).astype(np.float64)
        fps = np.where(has_truth, (held & ~near).sum(-1), held.sum(-1)).astype(np.float64)
    else:
        fns = (has_truth & ~has_picks).astype(np.float64)
        fps = (has_picks & ~(has_truth & hit)).astype(np.float64)
    return tps.sum(0), fps.sum(0), fns.sum(0), tps, fps, fns


def task0_residuals(truth, count, peak, start_sample, sampling_rate=TASK0_SAMPLING_RATE, method=0):
    """``compute_residuals`` (eval_taks0.py:326-353) for one phase: per threshold the residuals ``(pick - onset) /
    sampling_rate`` in seconds of the targets that have an onset and picks, in target order -- every pick (method 0), or per
    target the pick closest to the onset, the earlier of two equally close (method 1).  Returns a list of NT float64 arrays."""
    if method not in (0, 1):
        raise ValueError("method must be 0 or 1")
    truth = np.asarray(truth, np.float64)
    picks, held = _picks(count, peak, start_sample)
    held = held & ~np.isnan(truth)[:, None, None]
    res = (picks - truth[:, None, None]) / sampling_rate
    out = []
    for j in range(held.shape[1]):
        if method == 0:
            out.append(res[:, j][held[:, j]])
        else:
            some = held[:, j].any(-1)
            closest = np.argmin(np.where(held[:, j], np.abs(res[:, j]), np.inf), axis=-1)
            out.append(res[np.arange(len(truth)), j, closest][some])
    return out


TASK0_RESIDUAL_KEYS = ("mean", "median", "std", "MAE", "MAD", "out", "modified_mean", "modified_median", "modified_std",
                       "modified_RMSE", "modified_MAE", "modified_MAD", "modified_mean2", "modified_median2", "modified_std2",
                       "modified_RMSE2", "modified_MAE2", "modified_MAD2")


def _residual_stats(r):
    """The eighteen residual statistics of eval_taks0.py:605-641, in TASK0_RESIDUAL_KEYS' order; None each without residuals.
    "modified": residuals clipped to +-1 s; "modified...2": residuals beyond +-1 s (and at it) left out."""
    if len(r) == 0:
        return dict.fromkeys(TASK0_RESIDUAL_KEYS)
    mad = lambda a: np.median(np.abs(a - np.median(a)))
    clipped = np.clip(r, -1, 1)
    inside = r[(r > -1) & (r < 1)]
    values = (np.mean(r), np.median(r), np.std(r, ddof=1), np.mean(np.abs(r)), mad(r), ((r < -1) | (r > 1)).sum() / r.size,
              np.mean(clipped), np.median(clipped), np.std(clipped, ddof=1), np.sqrt(np.mean(clipped**2)),
              np.mean(np.abs(clipped)), mad(clipped),
              np.mean(inside), np.median(inside), np.std(inside, ddof=1), np.sqrt(np.mean(inside**2)),
              np.mean(np.abs(inside)), mad(inside))
    return dict(zip(TASK0_RESIDUAL_KEYS, values))


def task0_metrics(p_truth, s_truth, count, peak, start_sample, prob_thres, tp_thre=0.5, count_tp_method=0, no_p=False,
                  no_s=False):
    """The reference's metric table (eval_taks0.py:497-782) from one sweep: ``count`` (n, 2, NT) and ``peak`` (n, 2, NT, K)
    as ``sweep_bank`` returns them, ``p_truth`` / ``s_truth`` from ``task0_truth``.  One dict per threshold with the
    reference's keys in its order: ``prob_thre``, ``tp_thre``, then per phase ``TP FP FN precision recall F1score`` and the
    eighteen residual statistics (None each when the phase has no residuals).  ``no_p`` / ``no_s`` leave that phase's keys
    out (choosing the targets without that phase is the caller's part; ``eval_task0`` does it).  0 / 0 and the ``ddof=1``
    deviation of one value are numpy's NaN with its RuntimeWarning, as in the reference."""
    if no_p and no_s:
        raise ValueError("no_p and no_s together leave nothing to score")
    count, peak = np.asarray(count), np.asarray(peak)
    if len(prob_thres) != count.shape[2]:
        raise ValueError(f"{len(prob_thres)} thresholds for counts of {count.shape[2]}")
    per_phase = {}
    for ph, (name, truth, skip) in enumerate((("p", p_truth, no_p), ("s", s_truth, no_s))):
        if not skip:
            per_phase[name] = (task0_counts(truth, count[:, ph], peak[:, ph], start_sample, tp_thre, method=count_tp_method),
                               task0_residuals(truth, count[:, ph], peak[:, ph], start_sample, method=count_tp_method))
    rows = []
    for j, thr in enumerate(prob_thres):
        row = {"prob_thre": thr, "tp_thre": tp_thre}
        for name, ((TP, FP, FN, _, _, _), residuals) in per_phase.items():
            tp, fp, fn = TP[j], FP[j], FN[j]
            precision, recall = tp / (tp + fp), tp / (tp + fn)
            stats = {"TP": tp, "FP": fp, "FN": fn, "precision": precision, "recall": recall,
                     "F1score": 2.0 * (precision * recall) / (precision + recall)}
            stats.update(_residual_stats(residuals[j]))
            row.update({f"{name}_{k}": v for k, v in stats.items()})
        rows.append(row)
    return rows


def task0_tnr(p_truth, s_truth, count, prob_thres):
    """The rows of ``eval_task0_true_negative_rate`` (eval_taks0.py:943-971) from one sweep: per threshold and phase, among
    the targets WITHOUT an onset, TN those without picks, FP those with picks (one per target), and TN / (TN + FP) -- NaN
    where the reference's integer division raises because no target is without an onset."""
    count = np.asarray(count)
    rows = []
    for j, thr in enumerate(prob_thres):
        row = {"prob_thre": thr}
        for ph, (name, truth) in enumerate((("p", p_truth), ("s", s_truth))):
            negative = np.isnan(np.asarray(truth, np.float64))
            tn, fp = int((negative & (count[:, ph, j] == 0)).sum()), int((negative & (count[:, ph, j] > 0)).sum())
            with np.errstate(invalid="ignore"):
                row.update({f"{name}_TN": tn, f"{name}_FP": fp, f"{name}_true_negative_rate": np.float64(tn) / np.float64(tn + fp)})
        rows.append(row)
    return rows


def opt_prob_metrics(dev_metrics, test_metrics):
    """``opt_prob_metrics`` (eval_taks0.py:1139-1172) on two ``task0_metrics`` tables (lists of rows, or DataFrames) over the
    same thresholds: per phase the row where the DEV F1 score is largest (``np.argmax``: the first such row, and a NaN
    counts as largest, as it does there), and that row of both tables.  Keys in the reference's order without its
    ``exp_name``: ``tp_thre``, ``p_opt_prob_thre``, ``s_opt_prob_thre``, ``test_p_*``, ``test_s_*``, ``dev_p_*``, ``dev_s_*``."""
    def table(t):
        if hasattr(t, "to_dict") and not isinstance(t, dict):
            return t.to_dict("records")
        return list(t)

    dev, test = table(dev_metrics), table(test_metrics)
    best = {}
    for name in ("p", "s"):
        f1 = np.array([np.nan if r[f"{name}_F1score"] is None else r[f"{name}_F1score"] for r in dev], np.float64)
        best[name] = int(np.argmax(f1))
    result = {"tp_thre": test[0]["tp_thre"], "p_opt_prob_thre": dev[best["p"]]["prob_thre"],
              "s_opt_prob_thre": dev[best["s"]]["prob_thre"]}
    for prefix, rows in (("test_", test), ("dev_", dev)):
        for name in ("p", "s"):
            result.update({prefix + k: v for k, v in rows[best[name]].items() if k[:2] == name + "_"})
    return result


def eval_task0(model, bank, targets, prob_thres=np.arange(0.1, 1.0, 0.1), tp_thre=0.5, count_tp_method=0, no_p=False,
               no_s=False, batch_size=1024, max_picks=8):
    """``eval_task0`` of the reference (eval_taks0.py:370-825) for one set of task targets in ONE pass -- one forward per
    window, every threshold swept on the GPU: ``targets`` (a DataFrame or a dict of arrays) holds ``trace`` (the bank index),
    ``start_sample`` and ``end_sample``.  ``no_p`` / ``no_s`` keep the targets whose trace has no P / no S onset and leave
    that phase out of the table.  Returns ``(metrics, targets_out)``: the ``task0_metrics`` rows, and a copy of the (kept)
    targets with ``p_pred_sample_thr{thr:.4f}`` / ``s_pred_sample_thr{thr:.4f}`` added per threshold, in that order: per
    target one int64 array of picks in trace samples.  Files and directories are the caller's."""
    from .generate import SteeredPlanner

    if no_p and no_s:
        raise ValueError("no_p and no_s together leave nothing to score")
    onsets = np.asarray(bank.onsets, np.float64).reshape(-1, 4)[np.asarray(targets["trace"], np.int64)]
    keep = np.ones(len(onsets), bool)
    if no_p:
        keep &= np.isnan(onsets[:, 0])
    if no_s:
        keep &= np.isnan(onsets[:, 2])
    if isinstance(targets, dict):
        out = {k: np.asarray(v)[keep] for k, v in targets.items()}
    else:
        out = targets[keep].copy()
    rows, borders = SteeredPlanner(bank, model.in_samples).plan(out)
    count, peak, _ = sweep_bank(model, bank, rows, borders, prob_thres, batch_size, max_picks)
    start = np.asarray(out["start_sample"]).astype(np.int64)
    p_truth, s_truth = task0_truth(bank, out)
    metrics = task0_metrics(p_truth, s_truth, count, peak, start, prob_thres, tp_thre, count_tp_method, no_p, no_s)
    for j, thr in enumerate(prob_thres):
        for ph, name in enumerate("ps"):
            out[f"{name}_pred_sample_thr{thr:.4f}"] = [peak[i, ph, j, : count[i, ph, j]].astype(np.int64) + start[i]
                                                      for i in range(len(start))]
    return metrics, out
