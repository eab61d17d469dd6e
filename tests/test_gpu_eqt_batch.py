"""GPU: EQTransformer's block-1 batch from a device-resident bank (csrc/batchgen.hip, vp_bank_make_batch_eqt): x and the
P / S rows bit-equal to vp_bank_make_batch on the same rows, everything within the bars of the float64 restatement
(tests/eqt_batch_restate.py), the detection row exactly the restated rule's -- also on rows built around the adversarial
onsets -- and ``WaveformBank.make_batch`` for a model with a detection row."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import eqt_batch_restate as R
from tests.test_gpu_generate import build_traces, check_batch, edge_rows
from volpick_amd import _lib
from volpick_amd import generate as G

pytestmark = pytest.mark.gpu

ADV_START, ADV_L = 3000, 12000  # the adversarial onsets, window-relative, sit in traces of ADV_L samples cut at ADV_START


@pytest.fixture(scope="module")
def setup():
    """The traces of test_gpu_generate.py and one trace per adversarial case without a fixed window; the edge rows and one
    row per adversarial trace."""
    traces, onsets = build_traces()
    n0 = len(traces)
    cases = [c for c in R.ADVERSARIAL_ONSETS if c[2] is None]
    rng = np.random.default_rng(5)
    for _, rel, _, _ in cases:
        traces.append(rng.normal(0.0, 3.0, (3, ADV_L)).astype(np.float32))
        onsets = np.vstack([onsets, np.asarray(rel) + ADV_START])  # (integers and halves: the sum is exact)
    rows = np.zeros(len(cases), G.PLAN_ROW)
    for i in range(len(cases)):
        rows[i] = (n0 + i, 0, ADV_START, 0, ADV_L)
    rows = np.concatenate([edge_rows(traces), rows])
    bank = G.WaveformBank(traces, {"P": onsets[:, :2], "S": onsets[:, 2:]})
    yield traces, onsets, bank, rows, n0
    bank.close()


def raw(name, h, rows, x, y, T, sigma=20.0, norm=_lib.VP_NORM_PEAK, lrows=(0, 1, 2), fixed=None, B=None):
    """vp_bank_make_batch (fixed is None) or vp_bank_make_batch_eqt on CUDA tensors: the return code."""
    lr = (C.c_int * 3)(*lrows)
    rows = np.ascontiguousarray(rows)
    args = [h, rows.ctypes.data_as(C.c_void_p), len(rows) if B is None else B, T, sigma, norm, lr]
    if name == "vp_bank_make_batch_eqt":
        args.append(fixed)
    args += [C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    return getattr(_lib.load(), name)(*args)


def batches_of(rows, B):
    """Every row in some batch of B: B >= len(rows) repeats them round, smaller B walks them."""
    n = len(rows)
    if B >= n:
        return [rows[np.arange(B) % n]]
    return [rows[(k + np.arange(B)) % n] for k in range(0, n, B)]


@pytest.mark.parametrize("B", [1, 7, 257])
@pytest.mark.parametrize("T", [7, 1025, 6000, 6144])
def test_kernel_matches_the_restatement_and_the_phasenet_kernel(setup, T, B):
    traces, onsets, bank, all_rows, _ = setup
    for k, rows in enumerate(batches_of(all_rows, B)):
        norm, lrows = (("peak", (0, 1, 2)), ("std", (2, 0, 1)))[(k + B + T) % 2]
        sigma = (10.0, 20.0)[k % 2]
        x = torch.full((B, 3, T), 7.0, device="cuda")
        y = torch.full((B, 3, T), 7.0, device="cuda")
        x0, y0 = torch.empty_like(x), torch.empty_like(y)
        assert raw("vp_bank_make_batch_eqt", bank.handle, rows, x, y, T, sigma, G._norm(norm), lrows, -1.0) == 0, _lib.last_error()
        assert raw("vp_bank_make_batch", bank.handle, rows, x0, y0, T, sigma, G._norm(norm), (0, 1, 2)) == 0, _lib.last_error()
        torch.cuda.synchronize()
        gx, gy = x.cpu().numpy(), y.cpu().numpy()
        # the window and the P / S rows: the bits of vp_bank_make_batch
        assert np.array_equal(gx.view(np.uint32), x0.cpu().numpy().view(np.uint32))
        py0 = y0.cpu().numpy()
        assert np.array_equal(gy[:, lrows[1]].view(np.uint32), py0[:, 0].view(np.uint32))
        assert np.array_equal(gy[:, lrows[2]].view(np.uint32), py0[:, 1].view(np.uint32))
        # ... all of it within the bars of the float64 restatement, the detection row exactly
        wx, wy = R.restate(traces, onsets, rows, T, sigma, norm, lrows)
        check_batch(gx, gy, wx, wy, norm)
        det = gy[:, lrows[0]]
        assert np.array_equal(det, wy[:, lrows[0]]), np.flatnonzero((det != wy[:, lrows[0]]).any(-1))
        assert set(np.unique(det)) <= {0.0, 1.0}


def test_adversarial_rows_give_the_slices_worked_out_by_hand(setup):
    """At T = 6000, by the hand-made slices, not through the restatement: the fused-multiply-add case ends at 582."""
    traces, onsets, bank, all_rows, n0 = setup
    T = 6000
    cases = [c for c in R.ADVERSARIAL_ONSETS if c[2] is None]
    rows = all_rows[-len(cases):]
    x = torch.empty((len(rows), 3, T), device="cuda")
    y = torch.empty_like(x)
    assert raw("vp_bank_make_batch_eqt", bank.handle, rows, x, y, T, fixed=-1.0) == 0, _lib.last_error()
    det = y[:, 0].cpu().numpy()
    for i, (name, _, _, (p0, p1)) in enumerate(cases):
        want = np.zeros(T)
        want[p0:p1] = 1
        assert np.array_equal(det[i], want), name
    assert cases[-1][3] == (0, 582) and det[len(cases) - 1].sum() == 582


def test_fixed_window(setup):
    """Every case of the list with its fixed window (those without one: 250.5 samples), and the edge rows, at two T."""
    traces, onsets, bank, all_rows, n0 = setup
    for T in (6000, 1025):
        for w in (250.5, 1000.0, 100.0, 0.0):
            x = torch.empty((len(all_rows), 3, T), device="cuda")
            y = torch.empty_like(x)
            assert raw("vp_bank_make_batch_eqt", bank.handle, all_rows, x, y, T, lrows=(1, 2, 0), fixed=w) == 0, _lib.last_error()
            _, wy = R.restate(traces, onsets, all_rows, T, 20.0, "peak", (1, 2, 0), fixed_window=w)
            gy = y.cpu().numpy()
            assert np.array_equal(gy[:, 1], wy[:, 1]) and np.abs(gy - wy).max() <= 1e-6
    # the list's fixed-window cases by their hand-made slices, through a bank of their own
    cases = [c for c in R.ADVERSARIAL_ONSETS if c[2] is not None]
    tr = [np.ones((3, ADV_L), np.float32)] * len(cases)
    ons = np.array([c[1] for c in cases]) + ADV_START
    small = G.WaveformBank(tr, {"P": ons[:, :2], "S": ons[:, 2:]})
    try:
        for i, (name, _, w, (p0, p1)) in enumerate(cases):
            row = np.zeros(1, G.PLAN_ROW)
            row[0] = (i, 0, ADV_START, 0, ADV_L)
            out = small.make_batch(row, SimpleNamespace(in_samples=6000, norm="std", labels=["Detection", "P", "S"]), 20,
                                   detection_fixed_window=w)
            want = np.zeros(6000)
            want[p0:p1] = 1
            assert np.array_equal(out["detections"][0, 0].cpu().numpy(), want), name
    finally:
        small.close()


def test_bad_arguments_launch_nothing(setup):
    traces, onsets, bank, all_rows, _ = setup
    good = all_rows[:3]
    T = 6000
    x = torch.full((3, 3, 6200), 12345.0, device="cuda")
    y = torch.full((3, 3, 6200), -777.0, device="cuda")
    bad_trace = good.copy()
    bad_trace[1]["trace"] = len(traces)
    for kw in (dict(T=6145), dict(T=0), dict(lrows=(0, 0, 2)), dict(lrows=(0, 1, 3)), dict(rows=bad_trace), dict(B=0),
               dict(fixed=float("nan")), dict(fixed=float("inf")), dict(sigma=0.0), dict(norm=2)):
        a = dict(rows=good, T=T, sigma=20.0, norm=_lib.VP_NORM_PEAK, lrows=(0, 1, 2), fixed=-1.0, B=None)
        a.update(kw)
        rc = raw("vp_bank_make_batch_eqt", bank.handle, a["rows"], x, y, a["T"], a["sigma"], a["norm"], a["lrows"], a["fixed"], a["B"])
        assert rc == -1 and _lib.last_error(), kw  # VP_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((x == 12345.0).all()) and bool((y == -777.0).all())
    assert raw("vp_bank_make_batch_eqt", bank.handle, good, x, y, T, fixed=-1.0) == 0  # the good rows still run
    torch.cuda.synchronize()
    assert not bool((x.ravel()[:3 * 3 * T] == 12345.0).any()) and not bool((y.ravel()[:3 * 3 * T] == -777.0).any())


def test_make_batch_with_a_detection_row_returns_three_views(setup):
    traces, onsets, bank, all_rows, _ = setup
    T = 6000
    eqt = SimpleNamespace(in_samples=T, norm="std", labels=["Detection", "P", "S"])
    out = bank.make_batch(all_rows, eqt, 20)
    B = len(all_rows)
    assert set(out) == {"X", "y", "detections"}
    assert out["X"].shape == (B, 3, T) and out["y"].shape == (B, 2, T) and out["detections"].shape == (B, 1, T)
    # views of one (B, 3, T) tensor in the order detection, P, S
    assert out["y"].data_ptr() == out["detections"].data_ptr() + 4 * T
    assert out["y"].stride() == out["detections"].stride() == (3 * T, T, 1)
    wx, wy = R.restate(traces, onsets, all_rows, T, 20.0, "std", (0, 1, 2))
    got = torch.cat([out["detections"], out["y"]], 1).cpu().numpy()
    check_batch(out["X"].cpu().numpy(), got, wx, wy, "std")
    assert np.array_equal(got[:, 0], wy[:, 0])
    # a PhaseNet model keeps today's result; augmented rows with a detection row are refused
    pn = bank.make_batch(all_rows, SimpleNamespace(in_samples=3001, norm="peak", labels="PSN"), 20)
    assert set(pn) == {"X", "y"} and pn["y"].shape == (B, 3, 3001)
    with pytest.raises(ValueError, match="augmented"):
        bank.make_batch(np.zeros(2, G.AUG_ROW), eqt, 20)
    with pytest.raises(ValueError):
        bank.make_batch(all_rows, SimpleNamespace(in_samples=3001, norm="peak", labels="PSN"), 20, detection_fixed_window=100)
