"""GPU: EQTransformer's validation loss on the device.  The float64 weighted-BCE kernel (csrc/bce.hip, vp_bce_loss) against
the longdouble truth at a-priori bars (tests/eqt_batch_restate.py); one validation batch from a bank on an EQTransformer
handle (vp_validate_eqt_begin / _bank / _end) against the truth on the predictions it returns; and
``EQTransformerLit.validate_bank`` against the host path.

The tests print their worst error / bar; DESIGN.md §7 records the figures observed."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import eqt_batch_restate as R
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd import generate as G
from volpick_amd.synthetic import synthetic_stream_array
from volpick_amd.train import EQTransformerLit, validate_batches_eqt

pytestmark = pytest.mark.gpu

T = 6000
SENTINEL = -12345.0


def bce(p, y, weights, head=True, per_window=True, batch=True, shape=None):
    """vp_bce_loss on CUDA tensors: (return code, heads (B, C) or None, per-window values or None, batch value or None)."""
    lib = _lib.load()
    B, Cc, Tt = shape or p.shape
    new = lambda n: torch.full((max(n, 1),), SENTINEL, dtype=torch.float64, device="cuda")
    hd, pw, bt = (new(B * Cc) if head else None), (new(B) if per_window else None), (new(1) if batch else None)
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.vp_bce_loss(0, ptr(p), ptr(y), B, Cc, Tt, None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)),
                         ptr(hd), ptr(pw), ptr(bt), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy() if t is not None else None
    return rc, host(hd), host(pw), (float(bt.cpu()[0]) if batch else None)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def ratios(heads, windows, batch, p, y, w):
    """The errors against the longdouble truth over their bars: (head, window, batch) maxima, each asserted <= 1 by the caller."""
    th, tw, tb, _ = R.bce_truth(p, y, w)
    hb, wb, bb = R.bars(p, y, w)
    return (np.abs(heads - th) / hb).max(), (np.abs(windows - tw) / wb).max(), abs(batch - tb) / bb


SHAPES = [(1, 3, 7), (3, 1, 5), (2, 3, 6000), (5, 3, 3001), (257, 3, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_is_within_the_bars_of_the_longdouble_truth(shape):
    """Every input kind at every shape: heads, window values and the batch value inside the a-priori bars, a second launch
    equal to the bit, and any output left out (the batch value alone has the same bits as beside the window values)."""
    B, Cc, _ = shape
    w = R.weights_for(Cc)
    for kind in R.INPUT_KINDS:
        p, y = R.make_inputs(kind, shape, seed=len(kind) + B)
        pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
        rc, hd, pw, bt = bce(pd, yd, w)
        assert rc == 0, _lib.last_error()
        hd = hd.reshape(B, Cc)
        rh, rw, rb = ratios(hd, pw, bt, p, y, w)
        print(f"{kind} {shape}: max err / bar: heads {rh:.3g}, windows {rw:.3g}, batch {rb:.3g}")
        assert rh <= 1 and rw <= 1 and rb <= 1, (kind, rh, rw, rb)
        rc2, hd2, pw2, bt2 = bce(pd, yd, w)
        assert rc2 == 0 and (bits(hd2) == bits(hd.ravel())).all() and (bits(pw2) == bits(pw)).all() and bits(bt2) == bits(bt)
        rc3, hd3, pw3, none = bce(pd, yd, w, batch=False)
        assert rc3 == 0 and none is None and (bits(pw3) == bits(pw)).all() and (bits(hd3) == bits(hd.ravel())).all()
        rc4, hd4, none, none2 = bce(pd, yd, w, per_window=False, batch=False)
        assert rc4 == 0 and none is None and none2 is None and (bits(hd4) == bits(hd.ravel())).all()
        if B <= 5:  # (one workgroup walks the windows: not the path for large batches)
            rc5, hd5, none, bt5 = bce(pd, yd, w, per_window=False)
            assert rc5 == 0 and none is None and bits(bt5) == bits(bt) and (bits(hd5) == bits(hd.ravel())).all()
            rc6, none, none2, bt6 = bce(pd, yd, w, head=False, per_window=False)
            assert rc6 == 0 and bits(bt6) == bits(bt)


def test_kernel_reads_p_and_y_of_different_alignment():
    """y four bytes further than p from a 16-byte boundary (no wide loads), and both 8 bytes off one: the same bars."""
    shape = (3, 3, 3001)
    p, y = R.make_inputs("sigmoid", shape, seed=9)
    w = R.WEIGHTS
    for off_p, off_y in ((0, 1), (2, 2), (3, 0)):
        pbuf = torch.empty(p.size + 4, dtype=torch.float32, device="cuda")
        ybuf = torch.empty(y.size + 4, dtype=torch.float32, device="cuda")
        pbuf[off_p:off_p + p.size] = torch.from_numpy(p.ravel()).cuda()
        ybuf[off_y:off_y + y.size] = torch.from_numpy(y.ravel()).cuda()
        rc, hd, pw, bt = bce(pbuf[off_p:], ybuf[off_y:], w, shape=shape)
        assert rc == 0, _lib.last_error()
        rh, rw, rb = ratios(hd.reshape(3, 3), pw, bt, p, y, w)
        assert rh <= 1 and rw <= 1 and rb <= 1, (off_p, off_y, rh, rw, rb)


def test_kernel_propagates_non_finite_values():
    p, y = R.make_inputs("sigmoid", (5, 3, 3001), seed=4)
    p[1, 2, 1234] = np.nan
    p[3, 0, 7] = np.inf   # log(1 - inf) is NaN
    p[4, 1, 9] = -0.25    # outside [0, 1]: log p is NaN
    y[0, 0, 3] = np.inf   # inf * log p = -inf, (1 - inf) * log(1 - p) = +inf: NaN
    w = R.WEIGHTS
    rc, hd, pw, bt = bce(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(), w)
    assert rc == 0
    hd = hd.reshape(5, 3)
    th, tw, tb, _ = R.bce_truth(p, y, w)
    assert np.array_equal(np.isnan(hd), np.isnan(th)) and np.isnan(hd).sum() == 4
    assert np.array_equal(np.isnan(pw), np.isnan(tw)) and np.isnan(pw[[0, 1, 3, 4]]).all() and np.isnan(bt) and np.isnan(tb)
    hb, wb, _ = R.bars(p, y, w)
    ok = ~np.isnan(th)
    assert (np.abs(hd - th)[ok] <= hb[ok]).all() and abs(pw[2] - tw[2]) <= wb[2]


@pytest.mark.parametrize("bad", [dict(B=0), dict(C=0), dict(C=9), dict(T=0), dict(weights=None), dict(weights=(0.05, float("nan"), 0.55)),
                                 dict(p=None), dict(y=None)])
def test_kernel_argument_errors_launch_nothing(bad):
    p = torch.full((2, 8, 64), 0.3, device="cuda")
    a = dict(B=2, C=3, T=64, weights=R.WEIGHTS, p=p, y=p)
    a.update(bad)
    if a["C"] == 9:
        a["weights"] = np.ones(9)
    rc, hd, pw, bt = bce(a["p"], a["y"], a["weights"], shape=(a["B"], a["C"], a["T"]))
    assert rc == -1 and _lib.last_error()  # VP_ERR_INVALID
    assert (hd == SENTINEL).all() and (pw == SENTINEL).all() and bt == SENTINEL


# ---------------------------------------------------------------------------------------------------------- bank path
def eqt_bank(n=40, seed=21):
    """n traces with L from 3000 to 14000 (some shorter than a window), a P in each, an S in four of five."""
    rng = np.random.default_rng(seed)
    traces, ps, ss = [], [], []
    for i, L in enumerate(np.linspace(3000, 14000, n).astype(int)):
        x, p, s = synthetic_stream_array(int(L), seed=seed * 100003 + i, n_events=1)
        traces.append(np.ascontiguousarray(x * rng.uniform(0.1, 100.0), np.float32))
        ps.append(float(p[0]))
        ss.append(float(s[0]) if i % 5 else np.nan)
    return G.WaveformBank(traces, {"P": ps, "S": ss})


@pytest.fixture(scope="module")
def setup():
    bank = eqt_bank()
    model = EQTransformer.from_pretrained("volpick").cuda()
    yield bank, model, EQTransformerLit(model=model)
    bank.close()


def planned_rows(lit, bank, B, seed):
    return lit.window_planner(bank, B, seed=seed).plan(np.random.default_rng(seed).integers(0, bank.n_traces, B))


def stacked(model, batch):
    """(p, y): the model's three outputs and the batch's labels as (B, 3, T) arrays in the order detection, P, S."""
    p = torch.stack(model(batch["X"]), 1).cpu().numpy()
    y = torch.cat([batch["detections"], batch["y"]], 1).cpu().numpy()
    return p, y


@pytest.mark.parametrize("B", [1, 5, "max_batch + 1"])
def test_one_batch_from_a_bank(setup, B):
    """Window, head and batch losses within the bars of the truth on the predictions handed back and the labels of
    ``make_batch``; the predictions are bit-equal to ``model(batch["X"])`` (observed difference: 0), also across the chunk
    boundary, where B = max_batch + 1 leaves a chunk of one window."""
    bank, model, lit = setup
    if B == "max_batch + 1":
        B = model._max_batch + 1
    rows = planned_rows(lit, bank, B, seed=B)
    batch, window, heads, preds = validate_batches_eqt(model, bank, [rows], 20, predictions=True)
    made = bank.make_batch(rows, model, 20)
    direct, y = stacked(model, made)
    p = preds[0].cpu().numpy()
    assert batch.shape == (1,) and window.shape == (B,) and heads.shape == (B, 3) and p.shape == (B, 3, T)
    assert (B < 5 or y[:, 0].any()) and set(np.unique(y[:, 0])) <= {0.0, 1.0}
    rh, rw, rb = ratios(heads, window, batch[0], p, y, R.WEIGHTS)
    diff = np.abs(direct - p).max()
    print(f"B={B}: max err / bar: heads {rh:.3g}, windows {rw:.3g}, batch {rb:.3g}; max|pred - model(X)| = {diff:.3g}")
    assert np.isfinite(window).all() and (window > 0).all()
    assert rh <= 1 and rw <= 1 and rb <= 1
    assert (direct.view(np.uint32) == p.view(np.uint32)).all(), diff


def test_a_pass_of_five_batches_equals_five_passes(setup):
    bank, model, lit = setup
    sizes = [5, 16, 1, 9, 3]
    plans = [planned_rows(lit, bank, B, seed=50 + i) for i, B in enumerate(sizes)]
    batch, window, heads = validate_batches_eqt(model, bank, plans, 20)
    assert batch.shape == (5,) and window.shape == (sum(sizes),) and heads.shape == (sum(sizes), 3)
    off = 0
    for rows, b in zip(plans, batch):
        one_b, one_w, one_h = validate_batches_eqt(model, bank, [rows], 20)
        assert bits(one_b[0]) == bits(b)
        assert (bits(one_w) == bits(window[off:off + len(rows)])).all() and (bits(one_h) == bits(heads[off:off + len(rows)])).all()
        off += len(rows)
    # the weights and the fixed window reach the kernels
    b2, w2, h2 = validate_batches_eqt(model, bank, plans[:1], 20, loss_weights=(1.0, 0.0, 0.0))
    assert (bits(h2) == bits(heads[:5])).all() and np.abs(w2 - heads[:5, 0]).max() <= 4 * R.U * np.abs(w2).max()
    b3, w3, h3 = validate_batches_eqt(model, bank, plans[:1], 20, detection_fixed_window=300)
    assert (bits(h3[:, 1:]) == bits(heads[:5, 1:])).all() and (h3[:, 0] != heads[:5, 0]).any()


def test_refused_calls_append_nothing_and_other_passes_stay_open(setup):
    bank, model, lit = setup
    lib = _lib.load()
    h = model._ensure_handle()
    rows = planned_rows(lit, bank, 4, seed=1)
    lrows = (C.c_int * 3)(0, 1, 2)
    w = (C.c_double * 3)(*R.WEIGHTS)

    def call(r, weights=w, lr=lrows):
        return lib.vp_validate_eqt_bank(h, bank.handle, r.ctypes.data_as(C.c_void_p), len(r), 20.0, G._norm(model.norm), lr, -1.0,
                                        weights, None)

    def end(cap_b=1, cap_w=8):
        nb, nw = C.c_longlong(), C.c_longlong()
        one, four, heads = np.full(1, SENTINEL), np.full(8, SENTINEL), np.full(24, SENTINEL)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc = lib.vp_validate_eqt_end(h, dp(one), cap_b, C.byref(nb), dp(four), dp(heads), cap_w, C.byref(nw))
        return rc, nb.value, nw.value, one, four, heads

    if lib.vp_validate_eqt_begin(h) == 0:  # (close whatever an earlier test left open)
        end()
    assert call(rows) == -1 and "vp_validate_eqt_begin" in _lib.last_error()  # no pass is open
    assert end()[0] == -1
    assert lib.vp_predict_begin(h) == 0  # a prediction pass of the same handle, open beside this one
    assert lib.vp_validate_eqt_begin(h) == 0
    bad = rows.copy()
    bad["trace"][2] = bank.n_traces
    assert call(bad) == -1 and "trace" in _lib.last_error()
    assert call(rows, lr=(C.c_int * 3)(0, 1, 1)) == -1
    assert call(rows, weights=(C.c_double * 3)(0.05, float("inf"), 0.55)) == -1
    assert call(rows, weights=None) == -1
    assert call(rows) == 0
    rc, nb, nw, one, four, heads = end()
    assert rc == 0 and (nb, nw) == (1, 4)  # the refused calls left nothing behind
    assert one[0] != SENTINEL and (four[:4] != SENTINEL).all() and (four[4:] == SENTINEL).all()
    assert (heads[:12] != SENTINEL).all() and (heads[12:] == SENTINEL).all()
    want = validate_batches_eqt(model, bank, [rows], 20)
    assert bits(one[0]) == bits(want[0][0]) and (bits(heads[:12]) == bits(want[2].ravel())).all()
    n = C.c_longlong(-1)
    assert lib.vp_predict_end(h, None, 0, C.byref(n)) == 0 and n.value == 0  # still open, and empty


def test_a_phasenet_handle_is_unsupported(setup):
    bank, _, lit = setup
    lib = _lib.load()
    h = PhaseNet.from_pretrained("volpick").cuda()._ensure_handle()
    assert lib.vp_validate_eqt_begin(h) == -4 and "EQTransformer" in _lib.last_error()  # VP_ERR_UNSUPPORTED
    rows = planned_rows(lit, bank, 2, seed=1)
    assert lib.vp_validate_eqt_bank(h, bank.handle, rows.ctypes.data_as(C.c_void_p), 2, 20.0, 0, (C.c_int * 3)(0, 1, 2), -1.0,
                                    (C.c_double * 3)(*R.WEIGHTS), None) == -4


def test_validate_bank_equals_the_host_path(setup):
    """Batch by batch within twice the batch bar (the device's rounding and the host's own float64 rounding), for the
    planner form, the one-array form and the list form."""
    val, model, lit = setup
    got, window = lit.validate_bank(val, lit.window_planner(val, 16, seed=3), per_window=True)
    plans = list(lit.window_planner(val, 16, seed=3).validation())
    assert len(got) == len(plans) == 3 and window.shape == (40,)  # 16 + 16 + 8: the partial batch is kept
    worst = 0.0
    for g, rows in zip(got, plans):
        b = lit.make_batch(val, rows)
        loss = lit.validation_step(b)
        bar = R.bars(*stacked(model, b), R.WEIGHTS)[2]
        worst = max(worst, abs(g - loss) / (2 * bar))
        assert abs(g - loss) <= 2 * bar, (g, loss)
    print(f"max |device - host| / (2 batch bar) = {worst:.3g}")
    one = lit.validate_bank(val, plans[0])  # one array of rows is one batch: the pass's first
    assert len(one) == 1 and bits(one[0]) == bits(got[0]) and bits(lit.validate_bank(val, [plans[0]])[0]) == bits(got[0])
    assert [bits(v) for v in lit.validate_bank(val, plans)] == [bits(v) for v in got]


def test_the_two_released_weight_sets_score_differently(setup):
    val, model, lit = setup
    other = EQTransformerLit(model=EQTransformer.from_pretrained("volpick_95train"))
    plans = list(lit.window_planner(val, 20, seed=7).validation())
    a, b = np.array(lit.validate_bank(val, plans)), np.array(other.validate_bank(val, plans))
    print(f"volpick {a.mean():.6f}, volpick_95train {b.mean():.6f}")
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a > 0).all() and (b > 0).all() and (a != b).all()
