"""GPU: task 0 on the device.  The sweep kernel (csrc/sweep.hip, vp_sweep_windows) against the numpy restatement
(tests/task0_restate.py) on constructed probabilities, bit for bit, for both models' window lengths; its agreement with
vp_pick_windows and ``evaluate_windows``; the pass over a waveform bank (vp_sweep_begin / _bank / _end) against the
restatement on the probabilities of the same windows; ``evaluate.eval_task0``."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import volpick_amd as va
from tests import task0_restate as R
from tests.test_gpu_predict import direct, mixed_bank
from volpick_amd import _lib
from volpick_amd import evaluate as E
from volpick_amd import generate as G
from volpick_amd.synthetic import synthetic_windows

pytestmark = pytest.mark.gpu

SENTINEL = -77
GUARD = 3  # windows' worth of room behind every output array that no call may write to
B_ADV = 37


@pytest.fixture(scope="module")
def models():
    """name -> (model with max_batch = 8, so that a batch of 30 windows takes the chunked path; T; (p_row, s_row))."""
    out = {}
    for name, cls in (("phasenet", va.PhaseNet), ("eqtransformer", va.EQTransformer)):
        m = cls.from_pretrained("volpick")
        m._max_batch = 8
        m.cuda()
        out[name] = (m, m.in_samples, E._sweep_rows(m))
    return out


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sweep_on_gpu(model, prob, mem, rows, lo, hi, on, off, K, with_value=True, B=None, n_rows=None, NT=None):
    """vp_sweep_windows -> (return code, (count, peak, value or None)); the arrays are pre-filled with SENTINEL, carry GUARD
    windows of room behind the B the call is told about, and the room is checked."""
    lib = _lib.load()
    nb = len(prob) if B is None else B
    nt = NT if NT is not None else len(on if on is not None else off)
    room, k = max(nb, 1) + GUARD, max(K, 1)
    count = np.full((room, 2, max(nt, 1)), SENTINEL, np.int32)
    peak = np.full((room, 2, max(nt, 1), k), SENTINEL, np.int32)
    value = np.full((room, 2, max(nt, 1), k), SENTINEL, np.float32) if with_value else None
    keep = torch.from_numpy(np.array(prob)).cuda() if mem == _lib.VP_MEM_DEVICE else np.ascontiguousarray(prob)
    p = keep.data_ptr() if mem == _lib.VP_MEM_DEVICE else keep.ctypes.data
    if mem == _lib.VP_MEM_DEVICE:
        torch.cuda.synchronize()
    lo32, hi32 = (None if a is None else np.ascontiguousarray(a, np.int32) for a in (lo, hi))
    on32, off32 = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (on, off))
    rc = lib.vp_sweep_windows(model._ensure_handle(), C.c_void_p(p), mem, nb, prob.shape[1] if n_rows is None else n_rows, *rows,
                              ptr(lo32), ptr(hi32), ptr(on32), ptr(off32), nt, K, ptr(count), ptr(peak), ptr(value))
    used = nb if rc == 0 else 0
    for a in (count, peak) + ((value,) if with_value else ()):
        assert (a[used:] == SENTINEL).all(), "written outside the windows' slots"
    return rc, (count[:used], peak[:used], None if value is None else value[:used])


# (NT, K, value kept): the reference's grid with the default room; one threshold; the widest sweep; and the corners between
SHAPES = [(9, 8, True), (9, 8, False), (1, 1, True), (32, 64, True), (32, 1, False), (1, 64, False), (9, 64, True)]


@pytest.mark.parametrize("mem", [_lib.VP_MEM_HOST, _lib.VP_MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_constructed_probabilities_equal_the_restatement(models, name, mem):
    model, T, rows = models[name]
    on, off = R.thresholds(R.WIDE_GRID)
    for borders in (True, False):
        prob, lo, hi, wide = R.adversarial_case(T, B_ADV, 0, *rows, borders=borders)
        assert (wide[0][:, :, :9] > 8).any() and (wide[0] > 64).any() and (wide[0] == 0).any()  # counts above K are in it
        for NT, K, with_value in SHAPES if borders else SHAPES[:4]:
            rc, got = sweep_on_gpu(model, prob, mem, rows, *((lo, hi) if borders else (None, None)), on[:NT], off[:NT], K, with_value)
            assert rc == 0, _lib.last_error()
            want = R.narrowed(wide, NT, K)
            assert (got[2] is None) == (not with_value)
            assert R.same(got, want), (borders, NT, K, [b for b in range(B_ADV) if not R.same(tuple(
                None if g is None else g[b:b + 1] for g in got), tuple(w[b:b + 1] for w in want))])
            # the contract, spelled out: slots behind the count hold -1 / 0, the kept picks ascend and are the K lowest
            held = np.arange(K) < got[0][..., None]
            assert (got[1][~held] == -1).all() and (got[1][held] >= 0).all()
            assert got[2] is None or (got[2][~held] == 0).all()
            assert (np.diff(np.where(held, got[1], np.iinfo(np.int32).max), axis=-1) >= 0).all()
            assert (np.diff(got[1], axis=-1)[held[..., 1:]] > 0).all()
    # B = 1: one window per launch, every row kind and every border case once
    prob, lo, hi, wide = R.adversarial_case(T, B_ADV, 0, *rows, borders=True)
    want = R.narrowed(wide, 9, 8)
    for b in range(len(R.ROW_KINDS)):
        rc, got = sweep_on_gpu(model, prob[b:b + 1], mem, rows, lo[b:b + 1], hi[b:b + 1], on[:9], off[:9], 8)
        assert rc == 0 and R.same(got, tuple(w[b:b + 1] for w in want)), b


def test_other_rows_and_a_second_seed(models):
    """Five rows with the two somewhere among them, S in front of P too; and the batch of another seed."""
    model, T, _ = models["phasenet"]
    on, off = R.thresholds(R.GRID)
    for rows in ((4, 1), (0, 3), (2, 4)):
        prob, lo, hi = R.adversarial_batch(T, 14, 7, *rows, n_rows=5)
        rc, got = sweep_on_gpu(model, prob, _lib.VP_MEM_HOST, rows, lo, hi, on, off, 8)
        assert rc == 0 and R.same(got, R.sweep(prob, *rows, on, off, 8, lo, hi)), rows


@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_refusals_leave_the_outputs_untouched(models, name):
    model, T, rows = models[name]
    prob = np.full((4, 3, T), 0.25, np.float32)
    prob[:, :, 100:110] = 0.5
    lo, hi = np.array([0, 10, 20, 30]), np.array([T, 300, 200, 300])
    on, off = R.thresholds([0.2, 0.4, 0.6])
    lib = _lib.load()

    def refused(**kw):
        a = dict(prob=prob, mem=_lib.VP_MEM_HOST, rows=rows, lo=lo, hi=hi, on=on, off=off, K=8, B=None, n_rows=None, NT=None)
        a.update(kw)
        rc, _ = sweep_on_gpu(model, a["prob"], a["mem"], a["rows"], a["lo"], a["hi"], a["on"], a["off"], a["K"], True, a["B"],
                             a["n_rows"], a["NT"])  # (checks that every array still holds the sentinel everywhere)
        assert rc == -1 and _lib.last_error(), kw  # VP_ERR_INVALID

    refused(B=0)
    refused(B=-3)
    refused(NT=0)
    refused(NT=33)
    refused(NT=-1)
    refused(K=0)
    refused(K=65)
    refused(K=-2)
    refused(rows=(3, 1))          # a row out of range
    refused(rows=(1, -1))
    refused(rows=(1, 1))          # the same row twice
    refused(n_rows=1)
    refused(n_rows=65)
    refused(lo=np.array([0, -1, 20, 30]))
    refused(hi=np.array([T, 300, T + 1, 300]))
    refused(hi=np.array([T, 10, 200, 300]))   # empty: hi == lo
    refused(hi=np.array([T, 300, 200, 29]))   # hi < lo
    refused(lo=None)              # one border array without the other
    refused(hi=None)
    refused(on=None)
    refused(off=None)
    refused(on=np.array([0.2, np.nan, 0.6], np.float32))
    refused(on=np.array([0.2, np.inf, 0.6], np.float32))
    refused(off=np.array([0.1, 0.2, -np.inf], np.float32))
    refused(off=np.array([0.1, 0.5, 0.3], np.float32))  # thr_off above thr_on
    refused(mem=7)                # neither host nor device memory
    h = model._ensure_handle()
    for null in ("h", "prob", "count", "peak"):
        count, peak = np.full((4, 2, 3), SENTINEL, np.int32), np.full((4, 2, 3, 8), SENTINEL, np.int32)
        a = dict(h=h, prob=ptr(prob), count=ptr(count), peak=ptr(peak))
        a[null] = None
        assert lib.vp_sweep_windows(a["h"], a["prob"], 0, 4, 3, *rows, None, None, ptr(on), ptr(off), 3, 8, a["count"], a["peak"],
                                    None) == -1 and _lib.last_error()
        assert (count == SENTINEL).all() and (peak == SENTINEL).all(), null
    rc, got = sweep_on_gpu(model, prob, _lib.VP_MEM_HOST, rows, lo, hi, on, off, 8)  # and the handle still works
    assert rc == 0 and R.same(got, R.sweep(prob, *rows, on, off, 8, lo, hi))
    assert got[0][:, :, 0].tolist() == [[1, 1]] * 4 and got[0][:, :, 1].tolist() == [[1, 1]] * 4 and (got[0][:, :, 2] == 0).all()
    # one run over the whole border at the two lower thresholds; its maximum starts at sample 100 of the window
    assert got[1][:, 0, 0, 0].tolist() == got[1][:, 1, 1, 0].tolist() == [100, 90, 80, 70]


@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_one_threshold_of_the_sweep_is_vp_pick_windows_sorted(models, name):
    model, T, rows = models[name]
    lib = _lib.load()
    prob, lo, hi, wide = R.adversarial_case(T, B_ADV, 0, *rows, borders=True)
    on, off = R.thresholds(R.WIDE_GRID)
    rc, (count, peak, value) = sweep_on_gpu(model, prob, _lib.VP_MEM_HOST, rows, lo, hi, on[:9], off[:9], 64)
    assert rc == 0
    compared = 0
    for ph, row in enumerate(rows):
        for j in (0, 2, 8):
            c1, p1, v1 = np.zeros(B_ADV, np.int32), np.zeros((B_ADV, 64), np.int32), np.zeros((B_ADV, 64), np.float32)
            assert lib.vp_pick_windows(model._ensure_handle(), ptr(np.ascontiguousarray(prob)), _lib.VP_MEM_HOST, B_ADV, 3, row,
                                       ptr(lo), ptr(hi), float(on[j]), float(off[j]), 64, ptr(c1), ptr(p1), ptr(v1)) == 0
            assert np.array_equal(c1, count[:, ph, j])
            for b in np.flatnonzero(c1 <= 64):
                order = np.argsort(p1[b, :c1[b]], kind="stable")
                assert np.array_equal(p1[b, :c1[b]][order], peak[b, ph, j, :c1[b]]), (ph, j, b)
                assert np.array_equal(v1[b, :c1[b]][order].view(np.uint32), value[b, ph, j, :c1[b]].view(np.uint32))
                compared += int(c1[b])
    assert compared > 100


@pytest.mark.parametrize("name,T", [("phasenet", 3001), ("eqtransformer", 6000)])
def test_sweep_windows_equals_evaluate_windows_at_every_threshold(models, name, T):
    model, _, rows = models[name]
    n = 21
    x = synthetic_windows(n, T, seed=5)
    xn = x - x.mean(-1, keepdims=True)
    xn = (xn / (np.abs(xn).max(-1, keepdims=True) + 1e-10)).astype(np.float32)
    rng = np.random.default_rng(5)
    borders = np.stack([rng.integers(0, 400, n), rng.integers(T - 600, T + 1, n)], 1)
    count, peak, value = E.sweep_windows(model, xn, borders, batch_size=16, max_picks=64, scores=True)
    assert count.shape == (n, 2, 9) and peak.shape == value.shape == (n, 2, 9, 64)
    assert (count.dtype, peak.dtype, value.dtype) == (np.int32, np.int32, np.float32)
    y = model._forward_raw(xn)
    on, off = R.thresholds(R.GRID)
    assert R.same((count, peak, value), R.sweep(y, *rows, on, off, 64, borders[:, 0], borders[:, 1]))
    assert count[:, :, 2].sum() > 0
    for j in (0, 2, 5):
        pp, ps, sp, ss = E.evaluate_windows(model, xn, borders, threshold=R.GRID[j], batch_size=16, max_picks=64)
        for ph, (pk, sc) in enumerate(((pp, ps), (sp, ss))):
            for i in range(n):
                k = count[i, ph, j]
                assert np.array_equal(pk[i], peak[i, ph, j, :k]) and np.array_equal(sc[i], value[i, ph, j, :k]), (j, ph, i)
    # [P_thresholds, S_thresholds], no scores, whole windows
    c2, p2, v2 = E.sweep_windows(model, xn[:5], None, thresholds=[[0.3, 0.6], [0.6, 0.1]], max_picks=64)
    c9, p9, _ = E.sweep_windows(model, xn[:5], None, max_picks=64)
    assert v2 is None and np.array_equal(c2[:, 0], c9[:, 0][:, [2, 5]]) and np.array_equal(c2[:, 1], c9[:, 1][:, [5, 0]])
    assert np.array_equal(p2[:, 1], p9[:, 1][:, [5, 0]])
    if count.max() > 1:
        with pytest.raises(RuntimeError, match="max_picks"):
            E.sweep_windows(model, xn, borders, max_picks=int(count.max()) - 1)


# ------------------------------------------------------------------------------------------------------------ the pass
@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_a_pass_over_a_bank_equals_the_restatement(models, name):
    model, T, rows2 = models[name]
    bank, lengths, targets = mixed_bank(T, seed=3)
    try:
        assert (lengths < T).sum() == 3
        rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        n = len(rows)
        assert 30 <= n <= 36 and {1000, 3000} <= set((borders[:, 1] - borders[:, 0]).tolist())
        y = direct(model, bank, rows)
        on, off = R.thresholds(R.GRID)
        want = R.sweep(y, *rows2, on, off, 8, borders[:, 0], borders[:, 1])
        assert want[0].max() <= 8 and want[0][:, :, 2].sum() > 0

        whole = E.sweep_bank(model, bank, rows, borders, batch_size=n, scores=True, predictions=True)  # B > max_batch: chunks
        assert R.same(whole[:3], want) and len(whole[3]) == 1
        assert np.array_equal(whole[3][0].cpu().numpy().view(np.uint32), y.view(np.uint32))  # pred_out_dev: what was swept
        split = E.sweep_bank(model, bank, rows, borders, batch_size=n // 2 + 1, scores=True, predictions=True)
        assert R.same(split[:3], want) and [len(p) for p in split[3]] == [n // 2 + 1, n - n // 2 - 1]
        assert R.same(E.sweep_bank(model, bank, rows, borders, batch_size=8, scores=True), want)   # no chunking
        again = E.sweep_bank(model, bank, rows, borders, batch_size=n)   # a second pass on the handle, values not kept
        assert again[2] is None and R.same(again, want)
        # without borders: whole windows; another K and grid
        full = E.sweep_bank(model, bank, rows[:5], None, thresholds=[0.2, 0.45], batch_size=5, max_picks=16, scores=True)
        assert R.same(full, R.sweep(y[:5], *rows2, *R.thresholds([0.2, 0.45]), 16))
    finally:
        bank.close()


@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_the_pass_refuses_bad_calls_and_shares_the_handle(models, name):
    """Refused calls in front of, between and behind two accepted batches, and a prediction pass opened, fed and closed in
    the middle: the sweep pass holds the eight windows of its two batches, those of each batch alone, and nothing else; the
    prediction pass holds what it holds alone."""
    model, T, rows2 = models[name]
    bank, _, targets = mixed_bank(T, seed=4)
    lib = _lib.load()
    h = model._ensure_handle()
    on, off = R.thresholds(R.GRID)
    try:
        all_rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        rows, lo, hi = all_rows[:4], np.ascontiguousarray(borders[:4, 0]), np.ascontiguousarray(borders[:4, 1])
        rows_b, lo_b, hi_b = all_rows[4:8], np.ascontiguousarray(borders[4:8, 0]), np.ascontiguousarray(borders[4:8, 1])
        norm = G._norm(model.norm)

        def call(r, lo, hi, norm=norm, rows2=rows2, bank_h=bank.handle, B=None):
            return lib.vp_sweep_bank(h, bank_h, ptr(r), ptr(lo), ptr(hi), len(r) if B is None else B, norm, *rows2, None)

        def refusals():
            bad = rows.copy()
            bad["trace"][1] = 12
            assert call(bad, lo, hi) == -1 and "trace" in _lib.last_error()
            bad = rows.copy()
            bad["hi"][2] += 1  # past the trace's end
            assert call(bad, lo, hi) == -1
            assert call(rows, lo, lo) == -1 and "border" in _lib.last_error()  # empty borders
            assert call(rows, lo, hi + T) == -1
            assert call(rows, lo - T, hi) == -1
            assert call(rows, lo, hi, norm=5) == -1
            assert call(rows, lo, hi, rows2=(1, 1)) == -1
            assert call(rows, lo, hi, rows2=(1, 3)) == -1
            assert call(rows, lo, hi, bank_h=None) == -1
            assert call(rows, lo, hi, B=0) == -1
            assert call(None, None, None, B=4) == -1
            assert call(rows, lo, None) == -1  # lo without hi

        assert call(rows, lo, hi) == -1 and "no pass is open" in _lib.last_error()
        for bad_begin in ((ptr(on), ptr(off), 0, 8), (ptr(on), ptr(off), 33, 8), (ptr(on), ptr(off), 9, 0), (ptr(on), ptr(off), 9, 65),
                          (None, ptr(off), 9, 8), (ptr(on), None, 9, 8), (ptr(off), ptr(on), 9, 8)):
            assert lib.vp_sweep_begin(h, *bad_begin, 1) == -1
            assert call(rows, lo, hi) == -1 and "no pass is open" in _lib.last_error()
        assert lib.vp_sweep_begin(h, ptr(on), ptr(off), 9, 8, 1) == 0
        refusals()
        assert call(rows, lo, hi) == 0
        refusals()
        # a prediction pass of the same handle in the middle of the sweep pass
        alone = E.predict_bank(model, bank, all_rows[8:14], borders[8:14])
        refusals()
        assert call(rows_b, lo_b, hi_b) == 0
        refusals()
        count = np.full((12, 2, 9), SENTINEL, np.int32)
        peak = np.full((12, 2, 9, 8), SENTINEL, np.int32)
        value = np.full((12, 2, 9, 8), SENTINEL, np.float32)
        nw = C.c_longlong()
        assert lib.vp_sweep_end(h, None, None, None, 1, C.byref(nw)) == -1  # room announced, no arrays: the pass stays open
        assert lib.vp_sweep_end(h, ptr(count), ptr(peak), ptr(value), 12, C.byref(nw)) == 0
        assert nw.value == 8 and all((a[8:] == SENTINEL).all() for a in (count, peak, value))
        assert lib.vp_sweep_end(h, ptr(count), ptr(peak), ptr(value), 12, C.byref(nw)) == -1  # the pass is closed
        for part, (r, b) in ((slice(0, 4), (rows, borders[:4])), (slice(4, 8), (rows_b, borders[4:8]))):
            assert R.same((count[part], peak[part], value[part]), E.sweep_bank(model, bank, r, b, scores=True))
        y = direct(model, bank, all_rows[:8])
        assert R.same((count[:8], peak[:8], value[:8]), R.sweep(y, *rows2, on, off, 8, borders[:8, 0], borders[:8, 1]))
        outside = E.predict_bank(model, bank, all_rows[8:14], borders[8:14])  # the prediction pass, with no sweep pass open
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(alone, outside))
        # values asked of a pass that did not keep them
        assert lib.vp_sweep_begin(h, ptr(on), ptr(off), 9, 8, 0) == 0 and call(rows, lo, hi) == 0
        assert lib.vp_sweep_end(h, ptr(count), ptr(peak), ptr(value), 12, C.byref(nw)) == -1 and (value[8:] == SENTINEL).all()
        assert lib.vp_sweep_end(h, ptr(count), ptr(peak), None, 12, C.byref(nw)) == 0 and nw.value == 4
    finally:
        bank.close()


# ------------------------------------------------------------------------------------------------------------ eval_task0
def test_eval_task0_returns_the_table_and_the_columns(models):
    model, T, rows2 = models["phasenet"]
    bank, _, targets = mixed_bank(T, seed=3)
    try:
        before = {k: np.array(v) for k, v in targets.items()}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # 0 / 0 at the thresholds nothing reaches: numpy's NaN, kept
            metrics, out = E.eval_task0(model, bank, targets, batch_size=16)
        assert out is not targets and list(targets) == list(before) and all(np.array_equal(targets[k], before[k]) for k in before)
        names = [f"{ph}_pred_sample_thr{thr:.4f}" for thr in R.GRID for ph in "ps"]
        assert list(out) == list(before) + names and names[0] == "p_pred_sample_thr0.1000" and names[-1] == "s_pred_sample_thr0.9000"
        rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        n = len(rows)
        on, off = R.thresholds(R.GRID)
        count, peak, _ = R.sweep(direct(model, bank, rows), *rows2, on, off, 8, borders[:, 0], borders[:, 1])
        start = targets["start_sample"]
        for j in range(9):
            for ph, name in enumerate("ps"):
                col = out[names[2 * j + ph]]
                assert len(col) == n and all(c.dtype == np.int64 for c in col)
                assert all(np.array_equal(col[i], peak[i, ph, j, :count[i, ph, j]] + start[i]) for i in range(n))
        p_truth, s_truth = E.task0_truth(bank, targets)
        holds = (targets["start_sample"] <= targets["phase_onset"]) & (targets["phase_onset"] < targets["end_sample"])
        assert np.array_equal(~np.isnan(p_truth), holds) and np.isnan(s_truth).all()
        assert len(metrics) == 9 and [m["prob_thre"] for m in metrics] == R.GRID.tolist()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = E.task0_metrics(p_truth, s_truth, count, peak, start, R.GRID)
        for got_row, want_row in zip(metrics, want):
            assert list(got_row) == list(want_row)
            for k in want_row:
                a, b = got_row[k], want_row[k]
                assert (a is None and b is None) or a == b or (np.isnan(a) and np.isnan(b)), k
        for j, m in enumerate(metrics):
            # method 0, one onset at most per target: a target with an onset is a true positive or a false negative
            assert m["p_TP"] + m["p_FN"] == holds.sum() and m["s_TP"] + m["s_FN"] == 0
            assert m["s_FP"] == count[:, 1, j].sum()
        # the sanity bar of test_eval_tasks123...: half of the windows that hold the synthetic onset.  The torch-CPU oracle's own
        # probabilities of these windows, through the restatement, give 25 true positives of 25 at 0.3, so the bar stands.
        tp3 = metrics[2]["p_TP"]
        print(f"windows holding the onset: {holds.sum()}, true positives at 0.3: {tp3:.0f}")
        assert tp3 >= holds.sum() // 2
        # no_s keeps every target here (no trace has an S onset) and leaves the S keys out; no_p keeps none with an onset
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            only_p, out_p = E.eval_task0(model, bank, targets, no_s=True, count_tp_method=1, prob_thres=[0.3, 0.5])
        assert len(out_p["trace"]) == n and not any(k.startswith("s_") for k in only_p[0]) and only_p[0]["p_TP"] == tp3
        rows_tnr = E.task0_tnr(p_truth, s_truth, count, R.GRID)
        assert rows_tnr[2]["s_TN"] + rows_tnr[2]["s_FP"] == n and rows_tnr[2]["p_TN"] + rows_tnr[2]["p_FP"] == (~holds).sum()
    finally:
        bank.close()
