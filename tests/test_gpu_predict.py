"""GPU: the pick-benchmark tasks 1-3 on the device.  The per-window reduction kernel (csrc/predict.hip, vp_predict_windows)
against the numpy restatement (tests/predict_restate.py) on constructed probabilities, bit for bit; the pass over a
waveform bank (vp_predict_begin / _bank / _end) for both models against the restatement on the probabilities of the same
windows; ``evaluate.predict_windows`` against the restatement and the torch-CPU oracle; ``evaluate.eval_tasks123``."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import volpick_amd as va
from oracle.models import load_pretrained
from tests import predict_restate as R
from volpick_amd import _lib
from volpick_amd import evaluate as E
from volpick_amd import generate as G
from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the probability parity bar of tests/test_gpu_golden.py
SENTINEL = -77


@pytest.fixture(scope="module")
def models():
    """name -> (model with max_batch = 8, so that a batch of 30 windows takes the chunked path; T; rows; det_mode)."""
    out = {}
    for name, cls in (("phasenet", va.PhaseNet), ("eqtransformer", va.EQTransformer)):
        m = cls.from_pretrained("volpick")
        m._max_batch = 8
        m.cuda()
        out[name] = (m, m.in_samples) + tuple(E._predict_rows(m)[i] for i in (slice(0, 3), 3))
    return out


def reduce_on_gpu(model, prob, mem, rows, mode, lo, hi, B=None, n_rows=None):
    """vp_predict_windows -> (return code, records pre-filled with SENTINEL)."""
    lib = _lib.load()
    rec = np.zeros(max(B or len(prob), 1), E.RECORD)
    for k in rec.dtype.names:
        rec[k] = SENTINEL
    keep = torch.from_numpy(prob).cuda() if mem == _lib.VP_MEM_DEVICE else np.ascontiguousarray(prob)
    ptr = keep.data_ptr() if mem == _lib.VP_MEM_DEVICE else keep.ctypes.data
    if mem == _lib.VP_MEM_DEVICE:
        torch.cuda.synchronize()
    lo32, hi32 = (None if a is None else np.ascontiguousarray(a, np.int32) for a in (lo, hi))  # alive until the call returns
    as_ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.vp_predict_windows(model._ensure_handle(), C.c_void_p(ptr), mem, len(prob) if B is None else B,
                                prob.shape[1] if n_rows is None else n_rows, *rows, mode, as_ptr(lo32), as_ptr(hi32),
                                rec.ctypes.data_as(C.c_void_p))
    return rc, rec


@pytest.mark.parametrize("mem", [_lib.VP_MEM_HOST, _lib.VP_MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_constructed_probabilities_equal_the_restatement(models, name, mem):
    model, T, rows, mode = models[name]
    # B = 37: every border case and every row kind in one launch, two pairings of them
    for seed in (0, 5):
        prob, lo, hi = R.adversarial_batch(T, 37, seed, noise_row=rows[0], p_row=rows[1], s_row=rows[2])
        rc, rec = reduce_on_gpu(model, prob, mem, rows, mode, lo, hi)
        assert rc == 0, _lib.last_error()
        want = R.records(prob, *rows, mode, lo, hi)
        assert R.same_records(rec, want), [(b, rec[b], want[b]) for b in range(37) if not R.same_records(rec[b:b + 1], want[b:b + 1])]
    # B = 1: one window per launch, every border case once and the row kinds in turn
    n_cases = len(R.border_cases(T))
    for i in range(n_cases):
        kind = R.ROW_KINDS[i % len(R.ROW_KINDS)]
        a, e = R.border_cases(T)[i]
        prob = R.adversarial_window(kind, T, a, e, np.random.default_rng(i), *rows)[None]
        rc, rec = reduce_on_gpu(model, prob, mem, rows, mode, [a], [e])
        assert rc == 0 and R.same_records(rec, R.records(prob, *rows, mode, [a], [e])), (i, kind, a, e)
    # no borders: [0, T)
    prob, _, _ = R.adversarial_batch(T, 37, 3, noise_row=rows[0], p_row=rows[1], s_row=rows[2])
    rc, rec = reduce_on_gpu(model, prob, mem, rows, mode, None, None)
    assert rc == 0 and R.same_records(rec, R.records(prob, *rows, mode))


def test_other_rows_and_the_other_rule(models):
    """Five rows with the three somewhere among them, and each model's handle with the other model's rule."""
    model, T, _, _ = models["phasenet"]
    rng = np.random.default_rng(2)
    prob = rng.random((7, 5, T), dtype=np.float32)
    lo = rng.integers(0, 1000, 7).astype(np.int32)
    hi = (lo + rng.integers(1, 2000, 7)).astype(np.int32)
    for rows in ((4, 1, 3), (0, 4, 2)):
        for mode in (R.ONE_MINUS_NOISE, R.DET_ROW):
            rc, rec = reduce_on_gpu(model, prob, _lib.VP_MEM_HOST, rows, mode, lo, hi)
            assert rc == 0 and R.same_records(rec, R.records(prob, *rows, mode, lo, hi))


def test_the_sign_of_a_zero_maximum_is_that_of_the_lowest_index(models):
    """-0 == +0, so among zeros the lowest index wins and its value, sign included, is the maximum (torch's vectorised max
    may hand back either zero; the header pins this one)."""
    model, T, rows, mode = models["eqtransformer"]
    prob = np.full((2, 3, T), -1.0, np.float32)
    prob[0, :, 300], prob[0, :, 700] = -0.0, 0.0  # 700 - 300 puts the two zeros into different waves
    prob[1, :, 300], prob[1, :, 700] = 0.0, -0.0
    rc, rec = reduce_on_gpu(model, prob, _lib.VP_MEM_HOST, rows, mode, [0, 0], [T, T])
    assert rc == 0 and R.same_records(rec, R.records(prob, *rows, mode, [0, 0], [T, T]))
    assert rec["p_arg"].tolist() == [300, 300] and np.signbit(rec["p_max"]).tolist() == [True, False]
    assert np.signbit(rec["det"]).tolist() == [True, False]


@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_refusals_leave_the_records_untouched(models, name):
    model, T, rows, mode = models[name]
    prob = np.full((4, 3, T), 0.25, np.float32)
    lo, hi = np.array([0, 10, 20, 30]), np.array([T, 100, 200, 300])
    lib = _lib.load()

    def refused(**kw):
        a = dict(prob=prob, mem=_lib.VP_MEM_HOST, rows=rows, mode=mode, lo=lo, hi=hi, B=None, n_rows=None)
        a.update(kw)
        rc, rec = reduce_on_gpu(model, a["prob"], a["mem"], a["rows"], a["mode"], a["lo"], a["hi"], a["B"], a["n_rows"])
        assert rc == -1 and _lib.last_error(), kw  # VP_ERR_INVALID
        assert all((rec[k] == SENTINEL).all() for k in rec.dtype.names), kw

    refused(B=0)
    refused(B=-3)
    refused(rows=(3, 0, 1))       # a row out of range
    refused(rows=(-1, 0, 1))
    refused(rows=(2, 1, 1))       # not distinct
    refused(rows=(0, 0, 1))
    refused(n_rows=2)
    refused(mode=2)               # an unknown rule
    refused(lo=np.array([0, -1, 20, 30]))
    refused(hi=np.array([T, 100, T + 1, 300]))
    refused(hi=np.array([T, 10, 200, 300]))   # empty: hi == lo
    refused(hi=np.array([T, 100, 200, 29]))   # hi < lo
    refused(lo=None)              # one border array without the other
    refused(hi=None)
    refused(mem=7)                # neither host nor device memory
    h = model._ensure_handle()
    for null in ("h", "prob", "out"):  # a null handle, null probabilities, a null output
        rec = np.zeros(4, E.RECORD)
        for k in rec.dtype.names:
            rec[k] = SENTINEL
        a = dict(h=h, prob=prob.ctypes.data_as(C.c_void_p), out=rec.ctypes.data_as(C.c_void_p))
        a[null] = None
        assert lib.vp_predict_windows(a["h"], a["prob"], 0, 4, 3, *rows, mode, None, None, a["out"]) == -1 and _lib.last_error()
        assert all((rec[k] == SENTINEL).all() for k in rec.dtype.names), null
    rc, rec = reduce_on_gpu(model, prob, _lib.VP_MEM_HOST, rows, mode, lo, hi)  # and the handle still works
    want = np.float32(0.75) if mode == R.ONE_MINUS_NOISE else np.float32(0.25)
    assert rc == 0 and (rec["p_arg"] == 0).all() and (rec["det"] == want).all()


# ------------------------------------------------------------------------------------------------------------ the pass
def mixed_bank(T, seed):
    """12 synthetic traces of mixed length, three of them shorter than T, and steered targets with 10 s and 30 s borders."""
    lengths = [3 * T, T - 500, T, 2 * T + 333, T // 2, 4 * T, T + 1, 2 * T, T - 2, 3 * T, 2 * T, T + 999]
    waves, onsets = [], []
    for i, L in enumerate(lengths):
        x, p, _ = synthetic_stream_array(L, seed=seed * 1000 + i, n_events=1)
        waves.append(x.astype(np.float32) * (1 + i))
        onsets.append(float(p[0]))
    bank = G.WaveformBank(waves, {"P": onsets})
    targets = {"trace": [], "start_sample": [], "end_sample": []}
    for i, L in enumerate(lengths):
        p = int(onsets[i])
        for a, e in ((max(0, p - 500), min(L, max(0, p - 500) + 1000)),      # 10 s around the onset
                     (max(0, min(p - 1000, L - 3000)), min(L, max(0, min(p - 1000, L - 3000)) + 3000)),  # 30 s
                     (max(0, L - 1000), L)):                                 # the trace's last 10 s
            if e - a >= 1 and e - a <= T:
                for k, v in zip(targets, (i, a, e)):
                    targets[k].append(v)
    targets = {k: np.array(v) for k, v in targets.items()}
    targets["phase_onset"] = np.array(onsets)[targets["trace"]]
    return bank, np.array(lengths), targets


def direct(model, bank, rows):
    """The probabilities of the plan rows by the existing path: make_batch's X through _forward_raw."""
    as_model = SimpleNamespace(in_samples=model.in_samples, labels="PSN", norm=model.norm)  # (the labels it writes are unused)
    return model._forward_raw(bank.make_batch(rows, as_model, 20)["X"]).cpu().numpy()


@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_a_pass_over_a_bank_equals_the_restatement(models, name):
    model, T, rows3, mode = models[name]
    bank, lengths, targets = mixed_bank(T, seed=3)
    try:
        assert (lengths < T).sum() == 3
        rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        n = len(rows)
        assert 30 <= n <= 36 and {1000, 3000} <= set((borders[:, 1] - borders[:, 0]).tolist())
        y = direct(model, bank, rows)
        want = R.predict_step(R.records(y, *rows3, mode, borders[:, 0], borders[:, 1]))
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()

        def same(got):
            return (R.same_floats(got[0], want[0]) and R.same_floats(got[1], want[1]) and np.array_equal(got[2], want[2])
                    and np.array_equal(got[3], want[3]) and [g.dtype for g in got[:4]] == [np.float32, np.float32, np.int64, np.int64])

        whole = E.predict_bank(model, bank, rows, borders, batch_size=n, predictions=True)  # B > max_batch = 8: chunks
        assert same(whole) and len(whole[4]) == 1
        assert np.array_equal(whole[4][0].cpu().numpy().view(np.uint32), y.view(np.uint32))  # pred_out_dev: what was reduced
        split = E.predict_bank(model, bank, rows, borders, batch_size=n // 2 + 1, predictions=True)  # two batches of one pass
        assert same(split) and [len(p) for p in split[4]] == [n // 2 + 1, n - n // 2 - 1]
        assert same(E.predict_bank(model, bank, rows, borders, batch_size=8))   # no chunking
        assert same(E.predict_bank(model, bank, rows, borders, batch_size=n))   # a second pass on the handle: the same bits
        # without borders: whole windows
        full = E.predict_bank(model, bank, rows[:5], None, batch_size=5)
        w5 = R.predict_step(R.records(y[:5], *rows3, mode))
        assert R.same_floats(full[0], w5[0]) and np.array_equal(full[2], w5[2]) and np.array_equal(full[3], w5[3])
    finally:
        bank.close()


@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_the_pass_refuses_bad_rows_and_borders(models, name):
    """Refused calls in front of, between and behind two accepted batches: the pass holds the eight records of the two
    batches, those of each batch alone, and nothing else."""
    model, T, rows3, _ = models[name]
    bank, _, targets = mixed_bank(T, seed=4)
    lib = _lib.load()
    h = model._ensure_handle()
    try:
        all_rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        rows, lo, hi = all_rows[:4], np.ascontiguousarray(borders[:4, 0]), np.ascontiguousarray(borders[:4, 1])
        rows_b, lo_b, hi_b = all_rows[4:8], np.ascontiguousarray(borders[4:8, 0]), np.ascontiguousarray(borders[4:8, 1])

        def call(r, lo, hi, norm=G._norm(model.norm), rows3=rows3, bank_h=bank.handle):
            return lib.vp_predict_bank(h, bank_h, r.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p),
                                       hi.ctypes.data_as(C.c_void_p), len(r), norm, *rows3, None)

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
            assert call(rows, lo, hi, rows3=(0, 0, 1)) == -1
            assert call(rows, lo, hi, rows3=(0, 1, 3)) == -1
            assert call(rows, lo, hi, bank_h=None) == -1
            assert lib.vp_predict_bank(h, bank.handle, None, None, None, 4, G._norm(model.norm), *rows3, None) == -1
            assert lib.vp_predict_bank(h, bank.handle, rows.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), None, 4,
                                       G._norm(model.norm), *rows3, None) == -1  # lo without hi
            assert lib.vp_predict_bank(h, bank.handle, rows.ctypes.data_as(C.c_void_p), None, None, 0, G._norm(model.norm), *rows3, None) == -1

        assert call(rows, lo, hi) == -1 and "no pass is open" in _lib.last_error()
        assert lib.vp_predict_begin(h) == 0
        refusals()
        assert call(rows, lo, hi) == 0
        refusals()
        assert call(rows_b, lo_b, hi_b) == 0
        refusals()
        rec = np.zeros(12, E.RECORD)
        for k in rec.dtype.names:
            rec[k] = SENTINEL
        nw = C.c_longlong()
        assert lib.vp_predict_end(h, None, 1, C.byref(nw)) == -1  # room announced, no array: refused, the pass stays open
        assert lib.vp_predict_end(h, rec.ctypes.data_as(C.c_void_p), 12, C.byref(nw)) == 0
        assert nw.value == 8 and all((rec[k][8:] == SENTINEL).all() for k in rec.dtype.names)
        assert lib.vp_predict_end(h, rec.ctypes.data_as(C.c_void_p), 12, C.byref(nw)) == -1  # the pass is closed
        got = E._scores(rec[:8])
        for part, (r, b) in ((slice(0, 4), (rows, borders[:4])), (slice(4, 8), (rows_b, borders[4:8]))):
            alone = E.predict_bank(model, bank, r, b)
            assert R.same_floats(got[0][part], alone[0]) and R.same_floats(got[1][part], alone[1])
            assert np.array_equal(got[2][part], alone[2]) and np.array_equal(got[3][part], alone[3])
    finally:
        bank.close()


# ------------------------------------------------------------------------------------------- predict_windows, eval_tasks123
@pytest.mark.parametrize("name,T", [("phasenet", 3001), ("eqtransformer", 6000)])
def test_predict_windows_equals_the_restatement_and_agrees_with_the_oracle(models, name, T):
    model, _, rows3, mode = models[name]
    oracle = load_pretrained(name)
    oracle.norm_amp_per_comp = True  # the evaluation generator normalises per component, as in test_gpu_evaluate.py
    n = 37
    x = synthetic_windows(n, T, seed=5)
    xn = x - x.mean(-1, keepdims=True)
    xn = (xn / (np.abs(xn).max(-1, keepdims=True) + 1e-10)).astype(np.float32)
    rng = np.random.default_rng(5)
    borders = np.stack([rng.integers(0, 400, n), rng.integers(T - 600, T + 1, n)], 1)
    got = E.predict_windows(model, xn, borders, batch_size=16)
    assert [g.dtype for g in got] == [np.float32, np.float32, np.int64, np.int64] and all(g.shape == (n,) for g in got)
    y = model._forward_raw(xn)
    want = R.predict_step(R.records(y, *rows3, mode, borders[:, 0], borders[:, 1]))
    assert R.same_floats(got[0], want[0]) and R.same_floats(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    whole = E.predict_windows(model, xn[:3])
    assert R.same_floats(whole[0], R.predict_step(R.records(y[:3], *rows3, mode))[0])
    # the torch-CPU oracle's own probabilities through the reference's reductions
    with torch.no_grad():
        yo = oracle(torch.from_numpy(xn))
    yo = torch.stack(yo, 1).numpy() if isinstance(yo, tuple) else yo.numpy()
    ref = R.predict_step(R.records(yo, *rows3, mode, borders[:, 0], borders[:, 1]))
    err = np.abs(got[0] - ref[0]).max()
    print(f"{name}: max |score_detection - oracle| = {err:.3g}")
    assert err <= TOL
    for k, row in ((2, rows3[1]), (3, rows3[2])):
        peak = np.array([yo[i, row, s:e].max() for i, (s, e) in enumerate(borders)])
        clear = peak > 0.1  # a flat row has no stable argmax
        print(f"{name}: {'PS'[k - 2]} windows above 0.1: {clear.sum()} of {n}, max sample difference "
              f"{np.abs(got[k] - ref[k])[clear].max()}")
        assert clear.sum() >= 0.75 * n
        assert (np.abs(got[k] - ref[k])[clear] <= 1).all()


def test_eval_tasks123_adds_the_four_columns_in_order(models):
    model, T, rows3, mode = models["phasenet"]
    bank, _, targets = mixed_bank(T, seed=3)
    try:
        out = E.eval_tasks123(model, bank, targets, batch_size=16)
        assert out is not targets and "score_detection" not in targets
        rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        det, q, p, s = R.predict_step(R.records(direct(model, bank, rows), *rows3, mode, borders[:, 0], borders[:, 1]))
        assert R.same_floats(out["score_detection"], det) and R.same_floats(out["score_p_or_s"], q)
        assert np.array_equal(out["p_sample_pred"], p + targets["start_sample"])
        assert np.array_equal(out["s_sample_pred"], s + targets["start_sample"])
        # the wiring into the metrics: the windows that hold the synthetic P onset and whose pick lands within 0.5 s of it
        holds = (targets["start_sample"] <= targets["phase_onset"]) & (targets["phase_onset"] < targets["end_sample"])
        found = holds & (np.abs(out["p_sample_pred"] - targets["phase_onset"]) <= 50)
        print(f"windows holding the onset: {holds.sum()}, onset found within 0.5 s: {found.sum()}")
        assert found.sum() >= holds.sum() // 2
        table = {k: np.asarray(v)[found] for k, v in out.items()}
        table["phase_onset"] = table["p_sample_pred"].astype(np.float64)  # score the picks against themselves: residual 0
        table["phase_label"] = np.full(found.sum(), "P")
        table["sampling_rate"] = np.full(found.sum(), 100.0)
        stats = E.task23_metrics(table, table)
        assert stats["dev_P_mean_s"] == 0 and stats["test_P_rmse_s"] == 0 and stats["dev_P_out_s"] == 0
        table["phase_onset"] = np.asarray(targets["phase_onset"])[found]
        stats = E.task23_metrics(table, table)
        assert stats["dev_P_mae_s"] <= 0.5 and stats["dev_P_out_s"] == 0 and "dev_S_mean_s" not in stats
    finally:
        bank.close()
