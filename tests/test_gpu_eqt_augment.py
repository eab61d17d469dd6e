"""GPU: EQTransformer's stacked recipe generated from a device-resident waveform bank (csrc/batchgen.hip,
bank_aug_kernel<6, LABEL_DET>; vp_bank_make_batch_eqt_aug) against the float64 restatement of its records
(tests/eqt_augment_restate.py): planned batches, hand-made records, the null record against block 1's kernel, the shapes
at which the register tiling changes, invalid records, stream order; and the validation pass on such batches
(vp_validate_eqt_bank_aug, EQTransformerLit.validate_bank) against the loss of the same batches computed apart."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import eqt_augment_restate as R
from tests import eqt_batch_restate as RB
from tests.test_gpu_augment import CASES
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd import generate as G
from volpick_amd.train import EQTransformerLit, validate_batches_eqt

pytestmark = pytest.mark.gpu

T = 6000
SIGMA = 20
N_NOISE = 8
EQT = ["Detection", "P", "S"]
# the planner seed of the planned batches, chosen with the planner alone (it needs no GPU): the first seed at which every
# case has the slot under test active in at least 16 of its 64 windows (two_events is the scarce one: 18)
SEEDS = dict.fromkeys(CASES, 4)


def build_traces():
    """8 noise traces without picks, then 12 event traces of 14-18 k samples with P at 5000-7000 and S 700.25 behind it:
    one with an all-zero channel, one without an S, one without a pick."""
    rng = np.random.default_rng(17)
    traces, onsets = [], []
    for i in range(N_NOISE):
        L = 14000 + 500 * i
        traces.append((rng.standard_normal((3, L)) * (0.3 + i)).astype(np.float32))
        onsets.append([np.nan] * 4)
    for i in range(12):
        L = 14000 + 350 * i
        x = rng.standard_normal((3, L)).astype(np.float32) * (0.5 + i)
        p = 5000.0 + 181.3 * i
        x[:, int(p):int(p) + 600] *= 8
        ons = [p, np.nan, p + 700.25, np.nan]
        if i == 2:
            x[2] = 0.0  # an all-zero channel
        if i == 5:
            ons[2] = np.nan  # no S: no detection box
        if i == 7:
            ons = [np.nan] * 4  # no pick
        traces.append(x)
        onsets.append(ons)
    return traces, np.array(onsets)


def lit_for(norm="peak"):
    return EQTransformerLit(sigma=SIGMA, model=SimpleNamespace(in_samples=T, labels=EQT, norm=norm))


def planned(bank, B, seed, kw):
    """B augmented rows of `bank` (anything with lengths and onsets) planned with EQTransformer's windows."""
    n = len(bank.lengths)
    aug = G.Augmentation(event_traces=np.arange(N_NOISE, n), noise_traces=np.arange(0, N_NOISE), **kw)
    planner = lit_for().augmented_planner(bank, B, aug, seed=seed)
    return planner.plan(np.random.default_rng(seed).integers(0, n, B))


def active(case, rows):
    """How many windows have the slot under test of `case` active."""
    ev, nz = rows["event"]["kind"] != 0, rows["noise"]["kind"] != 0
    gap, gauss = rows["gap_hi"] > rows["gap_lo"], rows["gauss"] > 0
    return {
        "reference": (ev.any(1) | nz.any(1) | gap | gauss | (rows["cut"] < T)).sum(),
        "superimpose": (rows["event"]["kind"][:, 0] == G.AUG_BANK).sum(),
        "two_events": ev.all(1).sum(),
        "duplicate": (rows["event"]["kind"] == G.AUG_SELF).any(1).sum(),
        "noise": nz.all(1).sum(),
        "gauss": gauss.sum(),
        "gap": gap.sum(),
        "events_noise_gap": min(ev.any(1).sum(), (nz.any(1) | gauss).sum(), gap.sum()),
    }[case]


@pytest.fixture(scope="module")
def setup():
    traces, onsets = build_traces()
    bank = G.WaveformBank(traces, {"P": onsets[:, :2], "S": onsets[:, 2:]})
    yield traces, onsets, bank
    bank.close()


@pytest.fixture(scope="module")
def hand():
    traces = R.hand_traces()
    bank = G.WaveformBank(traces, {"P": R.HAND_ONSETS[:, :2], "S": R.HAND_ONSETS[:, 2:]})
    yield traces, R.HAND_ONSETS, bank
    bank.close()


def model_ns(norm, T_=T):
    return SimpleNamespace(in_samples=T_, labels=EQT, norm=norm)


def raw(bank, rows, x, y, T_=T, lrows=(0, 1, 2), fixed=-1.0, norm=_lib.VP_NORM_PEAK, sigma=float(SIGMA)):
    rows = np.ascontiguousarray(rows)
    return _lib.load().vp_bank_make_batch_eqt_aug(bank.handle, rows.ctypes.data_as(C.c_void_p), len(rows), T_, sigma, norm,
                                                  (C.c_int * 3)(*lrows), fixed, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))


def check(gx, gy, rows, traces, onsets, norm, T_=T, lrows=(0, 1, 2), fixed=None):
    """x within 4e-6 of the window's scale, P and S within 1e-6, the detection row exactly.  Equal records are restated
    once.

    The x bar is the one of test_gpu_augment.check at T = 3001 and needs no widening at T = 6000: both sides hold float64
    statistics (over 6000 samples their error is ~6000 * 2^-53 relative, far below fp32), so what separates them is the
    kernel's fp32 roundings -- one per normalised window and source, one per accumulation into x, one of the final
    quotient -- each 2^-24 = 6e-8 of a value of the order of the window's scale, and none grows with T."""
    gx, gy = gx.cpu().numpy().astype(np.float64), gy.cpu().numpy().astype(np.float64)
    i_det, i_p, i_s = lrows
    cache = {}
    worst = [0.0, 0.0]
    for b, rec in enumerate(rows):
        key = rec.tobytes()
        if key not in cache:
            cache[key] = R.execute_eqt(rec, traces, onsets, T_, SIGMA, norm, lrows, fixed)
        wx, wy = cache[key]
        scale = 1.0 if norm == "peak" else max(np.abs(wx).max(), 1e-30)
        ex = np.abs(gx[b] - wx).max() / scale
        ey = max(np.abs(gy[b, i_p] - wy[i_p]).max(), np.abs(gy[b, i_s] - wy[i_s]).max())
        worst = [max(worst[0], ex), max(worst[1], ey)]
        assert ex <= 4e-6, (b, ex, rec)
        assert ey <= 1e-6, (b, ey, rec)
        assert np.array_equal(gy[b, i_det], wy[i_det]), (b, np.flatnonzero(gy[b, i_det] != wy[i_det])[:8], rec)
    print(f"max x error / scale {worst[0]:.3g}, max P / S error {worst[1]:.3g}")


# ------------------------------------------------------------------------------------------------------ planned batches
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("norm", ["peak", "std"])
def test_kernel_matches_the_restatement(setup, case, norm):
    traces, onsets, bank = setup
    rows = planned(bank, 64, SEEDS[case], CASES[case])
    assert active(case, rows) >= 16, (case, active(case, rows))
    out = bank.make_batch_eqt_aug(rows, model_ns(norm), SIGMA)
    assert set(out) == {"X", "y", "detections"} and out["y"].shape == (64, 2, T) and out["detections"].shape == (64, 1, T)
    assert out["y"].data_ptr() == out["detections"].data_ptr() + 4 * T  # views of one tensor: detection, P, S
    torch.cuda.synchronize()
    check(out["X"], torch.cat([out["detections"], out["y"]], 1), rows, traces, onsets, norm)


def test_fixed_detection_window(setup):
    traces, onsets, bank = setup
    rows = planned(bank, 64, SEEDS["superimpose"], CASES["superimpose"])
    lit = EQTransformerLit(sigma=SIGMA, detection_fixed_window=1000, model=model_ns("peak"))
    out = lit.make_batch(bank, rows)  # dispatches on the rows' dtype
    torch.cuda.synchronize()
    y = torch.cat([out["detections"], out["y"]], 1)
    check(out["X"], y, rows, traces, onsets, "peak", fixed=1000)
    free = bank.make_batch_eqt_aug(rows, model_ns("peak"), SIGMA)
    assert not torch.equal(free["detections"], out["detections"]) and torch.equal(free["y"], out["y"])
    plain = lit.make_batch(bank, rows["primary"].copy())
    assert plain["X"].shape == (64, 3, T)
    with pytest.raises(ValueError, match="augmented"):
        bank.make_batch(rows, model_ns("peak"), SIGMA)  # make_batch itself keeps refusing them
    with pytest.raises(ValueError):
        bank.make_batch_eqt_aug(rows, SimpleNamespace(in_samples=3001, labels="PSN", norm="peak"), SIGMA)


# ---------------------------------------------------------------------------------------------------- hand-made records
@pytest.mark.parametrize("norm", ["peak", "std"])
def test_hand_made_records(hand, norm):
    traces, onsets, bank = hand
    recs, want, names = R.hand_records()
    out = bank.make_batch_eqt_aug(recs, model_ns(norm), SIGMA)
    torch.cuda.synchronize()
    det = out["detections"][:, 0].cpu().numpy()
    for i, name in enumerate(names):
        assert np.array_equal(det[i], want[i]), name  # the rows worked out by hand
    check(out["X"], torch.cat([out["detections"], out["y"]], 1), recs, traces, onsets, norm)
    y = out["y"].cpu().numpy()
    assert y[0, 0, 1500] == 1 and y[0, 1, 1500] == 1  # (a): P of the source on S of the primary, neither rescaled
    assert abs(y[4, 0, 1015] - np.exp(-225.0 / 800.0)) <= 1e-6  # (e): the maximum of the two Gaussians, whose sum is 1.51


def test_null_record_has_block_ones_label_bits(setup):
    traces, onsets, bank = setup
    lit = lit_for()
    prim = lit.window_planner(bank, 64, seed=4).plan(np.random.default_rng(4).integers(0, bank.n_traces, 64))
    recs = np.zeros(64, G.AUG_ROW)
    recs["primary"], recs["cut"] = prim, T
    for norm in ("peak", "std"):
        a = bank.make_batch_eqt_aug(recs, model_ns(norm), SIGMA)
        b = bank.make_batch(prim, model_ns(norm), SIGMA)
        assert torch.equal(a["y"].view(torch.int32), b["y"].view(torch.int32))
        assert torch.equal(a["detections"], b["detections"]) and bool(b["detections"].any())
        # x is normalised twice: the second pass moves it by roundings only
        assert float((a["X"] - b["X"]).abs().max()) <= 4e-6 * float(b["X"].abs().max())


# ------------------------------------------------------------------------------------- where the register tiling changes
def shape_records(traces, T_, B):
    """B records from six templates, each with a shifted event: sources from a bank window or the window itself, shifts of
    both signs, a cut, a gap, stacked noise and Gaussian noise."""
    def row(tr, start):
        return (tr, 0, start, 0, traces[tr].shape[1])

    d = max(T_ // 3, 1)
    t = np.zeros(6, G.AUG_ROW)
    t["cut"] = T_
    t[0]["primary"] = row(8, 4000)
    t[0]["event"][0] = (row(9, 4500), G.AUG_BANK, T_ // 10, d, 0.5)
    t[1]["primary"] = row(10, 5200)  # trace 10 has an all-zero channel
    t[1]["cut"] = T_ - T_ // 4
    t[1]["event"][0] = (row(11, traces[11].shape[1] - T_ // 2), G.AUG_BANK, 0, -d, 1.5)  # straddles the trace's end
    t[1]["event"][1] = (row(12, 5000), G.AUG_BANK, T_ // 5, min(2 * d, T_), 0.3)
    t[2]["primary"] = row(12, 4800)
    t[2]["event"][0] = ((0, 0, 0, 0, 0), G.AUG_SELF, T_ // 8, d, 2.0)
    t[2]["noise"][0] = (row(1, 3000), G.AUG_BANK, 0.1)
    t[2]["noise"][1] = (row(3, -T_ // 2), G.AUG_BANK, 0.02)  # straddles the trace's start
    t[3]["primary"] = row(13, 5500)  # no S
    t[3]["event"][0] = (row(14, 5600), G.AUG_BANK, 0, -1, 1.0)
    t[3]["gauss"], t[3]["noise_key"] = 0.1, 0x0123456789ABCDEF
    t[4]["primary"] = row(16, 6000)
    t[4]["event"][0] = (row(17, 6000), G.AUG_BANK, 0, -T_, 1.0)  # wholly outside
    t[4]["gap_lo"], t[4]["gap_hi"] = T_ // 7, T_ - T_ // 7
    t[5]["primary"] = row(18, 6100)
    t[5]["event"][0] = ((0, 0, 0, 0, 0), G.AUG_SELF, 0, 1, 0.75)
    t[5]["event"][1] = ((0, 0, 0, 0, 0), G.AUG_SELF, 0, 0, 0.25)  # unshifted: the box is dropped
    t[5]["gap_lo"], t[5]["gap_hi"] = T_ // 2, T_ // 2 + 1
    return t[np.arange(B) % 6]


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("T_", [1, 1023, 1025, 3073, 6144])
def test_shapes_and_label_orders(setup, T_, B):
    traces, onsets, bank = setup
    recs = shape_records(traces, T_, B)
    if B == 1:
        recs = shape_records(traces, T_, 6)[(T_ % 6):(T_ % 6) + 1]
    lrows = ((0, 1, 2), (2, 0, 1), (1, 2, 0))[(T_ + B) % 3]
    norm = ("peak", "std")[(T_ + B) % 2]
    x = torch.full((B, 3, T_), 7.0, device="cuda")
    y = torch.full((B, 3, T_), 7.0, device="cuda")
    assert raw(bank, recs, x, y, T_, lrows, norm=G._norm(norm)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    check(x, y, recs, traces, onsets, norm, T_, lrows)


def test_t_of_6145_is_refused(setup):
    traces, onsets, bank = setup
    recs = shape_records(traces, 6144, 2)
    x = torch.full((2, 3, 6145), 7.0, device="cuda")
    y = torch.full((2, 3, 6145), 7.0, device="cuda")
    assert raw(bank, recs, x, y, 6145) == -1 and "6144" in _lib.last_error()
    assert raw(bank, recs, x, y, 0) == -1
    torch.cuda.synchronize()
    assert bool((x == 7).all()) and bool((y == 7).all())


# ------------------------------------------------------------------------------------------------------ invalid records
def test_invalid_records_are_refused_and_leave_the_outputs_untouched(setup):
    traces, onsets, bank = setup
    good = shape_records(traces, T, 6)
    bad = []

    def variant(f):
        r = good.copy()
        f(r)
        bad.append(r)

    variant(lambda r: r[0]["event"].__setitem__(0, ((99, 0, 0, 0, 10), G.AUG_BANK, 0, 0, 1.0)))  # trace out of range
    variant(lambda r: r[1]["event"].__setitem__(0, ((10, 0, 0, 0, 10 ** 7), G.AUG_BANK, 0, 0, 1.0)))  # hi past the trace
    variant(lambda r: r[1]["event"].__setitem__(1, ((11, 0, 0, 0, 10), G.AUG_BANK, 0, T + 1, 1.0)))  # |shift| > T
    variant(lambda r: r[2]["event"].__setitem__(0, ((0, 0, 0, 0, 0), G.AUG_SELF, 0, 0, -1.0)))  # negative scale
    variant(lambda r: r[2]["noise"].__setitem__(0, ((1, 0, 0, 0, 10), G.AUG_BANK, np.inf)))  # non-finite scale
    variant(lambda r: r[3].__setitem__("gap_lo", 20) or r[3].__setitem__("gap_hi", 10))  # gap_lo > gap_hi
    variant(lambda r: r[3].__setitem__("cut", T + 1))
    variant(lambda r: r[0]["event"].__setitem__(1, ((0, 0, 0, 0, 0), G.AUG_NONE, 0, 5, 0.0)))  # unused, not zero
    variant(lambda r: r[0]["noise"].__setitem__(1, ((0, 0, 0, 0, 0), 3, 0.0)))  # kind out of range
    variant(lambda r: r[4].__setitem__("noise_key", 7))  # a key without Gaussian noise
    variant(lambda r: r[2]["event"].__setitem__(0, ((1, 0, 0, 0, 0), G.AUG_SELF, 0, 0, 1.0)))  # self with a row
    variant(lambda r: r[0]["event"].__setitem__(0, ((9, 0, 0, 0, 10), G.AUG_BANK, T + 1, 0, 1.0)))  # zero_before > T
    variant(lambda r: r[5]["primary"].__setitem__("lo", -1))
    x = torch.full((6, 3, T), 7.0, device="cuda")
    y = torch.full((6, 3, T), 7.0, device="cuda")
    for i, r in enumerate(bad):
        assert raw(bank, r, x, y) == -1 and _lib.last_error(), i  # VP_ERR_INVALID
        with pytest.raises(_lib.VolpickHipError):
            bank.make_batch_eqt_aug(r, model_ns("peak"), SIGMA)
    for fixed in (float("nan"), float("inf")):
        assert raw(bank, good, x, y, fixed=fixed) == -1 and "det_fixed_window" in _lib.last_error()
    assert raw(bank, good, x, y, lrows=(0, 1, 1)) == -1
    assert raw(bank, good, x, y, sigma=0.0) == -1
    assert raw(bank, good, x, y, norm=2) == -1
    with pytest.raises(ValueError):
        bank.make_batch_eqt_aug(good, model_ns("peak"), SIGMA, detection_fixed_window=float("inf"))
    torch.cuda.synchronize()
    assert bool((x == 7).all()) and bool((y == 7).all())
    assert raw(bank, good, x, y) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert not bool((x == 7).any()) and not bool((y == 7).any())


# --------------------------------------------------------------------------------------------------------- stream order
def test_a_batch_on_another_stream_is_read_on_that_stream(setup):
    """make_batch_eqt_aug enqueues on torch's current stream: a copy enqueued on that stream behind it sees the batch, with
    no device-wide wait in between."""
    traces, onsets, bank = setup
    rows = planned(bank, 64, SEEDS["events_noise_gap"], CASES["events_noise_gap"])
    want = bank.make_batch_eqt_aug(rows, model_ns("std"), SIGMA)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        got = bank.make_batch_eqt_aug(rows, model_ns("std"), SIGMA)
        hx = torch.empty(got["X"].shape, dtype=torch.float32, pin_memory=True)
        hy = torch.empty((64, 3, T), dtype=torch.float32, pin_memory=True)
        hx.copy_(got["X"], non_blocking=True)
        hy.copy_(torch.cat([got["detections"], got["y"]], 1), non_blocking=True)
        side.synchronize()  # this stream alone
    assert torch.equal(hx, want["X"].cpu())
    assert torch.equal(hy, torch.cat([want["detections"], want["y"]], 1).cpu())


# ------------------------------------------------------------------------------------------------------ validation pass
from tests.test_gpu_eqt_validate import bce, bits, ratios, stacked  # noqa: E402


@pytest.fixture(scope="module")
def net(setup):
    model = EQTransformer.from_pretrained("volpick").cuda()
    return model, EQTransformerLit(sigma=SIGMA, model=model)


def check_pass(model, lit, bank, plans):
    """One pass over `plans` (augmented and plan-row batches): per batch the predictions are the bits of the model's
    forward on the batch made apart, the head, window and batch values lie within the a-priori bars of the longdouble
    truth (the bar of tests/test_gpu_eqt_validate.py's plan-row pass) and within twice the bars of vp_bce_loss on the
    same tensors; and the pass equals its batches' own passes bit for bit."""
    batch, window, heads, preds = validate_batches_eqt(model, bank, plans, SIGMA, predictions=True)
    assert batch.shape == (len(plans),) and window.shape == (sum(map(len, plans)),)
    off = 0
    for k, rows in enumerate(plans):
        B = len(rows)
        made = lit.make_batch(bank, rows)
        direct, y = stacked(model, made)
        p = preds[k].cpu().numpy()
        assert (direct.view(np.uint32) == p.view(np.uint32)).all(), k
        h, w = heads[off:off + B], window[off:off + B]
        rh, rw, rb = ratios(h, w, batch[k], p, y, RB.WEIGHTS)
        print(f"batch {k} (B={B}, {'aug' if rows.dtype == G.AUG_ROW else 'plan'}): err / bar heads {rh:.3g}, windows {rw:.3g}, "
              f"batch {rb:.3g}")
        assert np.isfinite(w).all() and (w > 0).all() and rh <= 1 and rw <= 1 and rb <= 1
        rc, hd, pw, bt = bce(preds[k], torch.cat([made["detections"], made["y"]], 1).contiguous(), RB.WEIGHTS)
        assert rc == 0
        hb, wb, bb = RB.bars(p, y, RB.WEIGHTS)
        assert (np.abs(hd.reshape(B, 3) - h) <= 2 * hb).all() and (np.abs(pw - w) <= 2 * wb).all() and abs(bt - batch[k]) <= 2 * bb
        one_b, one_w, one_h = validate_batches_eqt(model, bank, [rows], SIGMA)
        assert bits(one_b[0]) == bits(batch[k]) and (bits(one_w) == bits(w)).all() and (bits(one_h) == bits(h)).all()
        off += B


def test_validation_pass_of_augmented_and_plan_row_batches(setup, net):
    traces, onsets, bank = setup
    model, lit = net
    a5 = planned(bank, 5, 31, CASES["events_noise_gap"])
    a40 = planned(bank, 40, 32, {})
    p7 = lit.window_planner(bank, 7, seed=33).plan(np.arange(7) + N_NOISE)
    assert (a5["event"]["kind"] != 0).any() and (a40["event"]["kind"] != 0).any()
    check_pass(model, lit, bank, [a5, p7, a40])


def test_validation_batch_larger_than_max_batch(setup, net):
    traces, onsets, bank = setup
    model, lit = net
    B = model._max_batch + 1
    check_pass(model, lit, bank, [planned(bank, B, 34, {})])


def test_validate_bank_with_an_augmented_planner_equals_the_host_path(setup, net):
    """The reference's validation pass: batch by batch within twice the batch bar of validation_step on the same batches
    (the bar of tests/test_gpu_eqt_validate.py's host route)."""
    traces, onsets, bank = setup
    model, lit = net
    aug = G.Augmentation(val_event_traces=np.arange(N_NOISE, bank.n_traces), val_noise_traces=np.arange(0, N_NOISE))
    got, window = lit.validate_bank(bank, lit.augmented_planner(bank, 8, aug, seed=3, validation=True), per_window=True)
    plans = list(lit.augmented_planner(bank, 8, aug, seed=3, validation=True).validation())
    assert len(got) == len(plans) == 3 and window.shape == (20,) and all(p.dtype == G.AUG_ROW for p in plans)
    assert sum((p["event"]["kind"] != 0).any() or (p["noise"]["kind"] != 0).any() or (p["gap_hi"] > 0).any() for p in plans)
    for g, rows in zip(got, plans):
        b = lit.make_batch(bank, rows)
        loss = lit.validation_step(b)
        bar = RB.bars(*stacked(model, b), RB.WEIGHTS)[2]
        assert abs(g - loss) <= 2 * bar, (g, loss, bar)
    assert [bits(v) for v in lit.validate_bank(bank, plans)] == [bits(v) for v in got]


def test_a_phasenet_handle_is_unsupported(setup):
    traces, onsets, bank = setup
    lib = _lib.load()
    h = PhaseNet.from_pretrained("volpick").cuda()._ensure_handle()
    rows = planned(bank, 2, 1, {})
    assert lib.vp_validate_eqt_bank_aug(h, bank.handle, rows.ctypes.data_as(C.c_void_p), 2, 20.0, 0, (C.c_int * 3)(0, 1, 2), -1.0,
                                        (C.c_double * 3)(*RB.WEIGHTS), None) == -4  # VP_ERR_UNSUPPORTED
    assert "EQTransformer" in _lib.last_error()
