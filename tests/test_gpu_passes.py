"""GPU: what the passes over a bank (vp_validate_*, vp_predict_*, vp_sweep_*) and vp_bank_make_batch keep from batch to
batch -- the staging ring of the plan rows, the batch scratch and the results arrays.  One pass long enough for the ring to
wrap, then a batch that outgrows the ring's slots, the scratch and the results, then a small one; three passes open on one
handle, their batches interleaved; and the same for the bank's own ring.  Every result is compared, bit for bit, with the
same batches run one at a time where nothing is carried over."""
import ctypes as C

import numpy as np
import pytest
import torch

import volpick_amd as va
from tests.test_gpu_generate import synthetic_bank
from tests.test_gpu_predict import direct, mixed_bank
from tests.test_gpu_validate import planned_rows
from volpick_amd import _lib
from volpick_amd import evaluate as E
from volpick_amd import generate as G
from volpick_amd.train import validate_batches

pytestmark = pytest.mark.gpu

MAX_BATCH = 8
RING = 8  # RowRing::N (csrc/batchgen.h)
# 2 N + 3 small batches: every slot is used twice and the ring wraps; 20 windows > max_batch: the slots, the scratch and the
# results regrow with the earlier results kept, and the forward runs in chunks; then a batch that fits what now stands
SIZES = [1 + i % 3 for i in range(2 * RING + 3)] + [20, 2]
SIGMA = 20
CLASSES = {"phasenet": va.PhaseNet, "eqtransformer": va.EQTransformer}


def fresh_model(name):
    """A model whose handle has run nothing: every capacity starts at zero."""
    m = CLASSES[name].from_pretrained("volpick")
    m._max_batch = MAX_BATCH
    return m.cuda()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def out_tensor(model, B):
    out = torch.empty((B, 3, model.in_samples), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return out


class PredictPass:
    def __init__(self, model, bank):
        self.model, self.bank, self.h, self.lib = model, bank, model._ensure_handle(), _lib.load()

    def begin(self):
        _lib.check(self.lib.vp_predict_begin(self.h), "vp_predict_begin")

    def feed(self, rows, borders):
        out = out_tensor(self.model, len(rows))
        lo, hi = np.ascontiguousarray(borders[:, 0], np.int32), np.ascontiguousarray(borders[:, 1], np.int32)
        _lib.check(self.lib.vp_predict_bank(self.h, self.bank.handle, ptr(rows), ptr(lo), ptr(hi), len(rows), G._norm(self.model.norm),
                                            *E._predict_rows(self.model)[:3], C.c_void_p(out.data_ptr())), "vp_predict_bank")
        return out

    def end(self, n):
        rec, nw = np.zeros(n, E.RECORD), C.c_longlong()
        _lib.check(self.lib.vp_predict_end(self.h, ptr(rec), n, C.byref(nw)), "vp_predict_end")
        assert nw.value == n
        return E._scores(rec)


class SweepPass(PredictPass):
    K = 8

    def begin(self):
        self.on, self.off, _ = E._sweep_grid(np.arange(0.1, 1.0, 0.1))
        _lib.check(self.lib.vp_sweep_begin(self.h, ptr(self.on), ptr(self.off), len(self.on), self.K, 1), "vp_sweep_begin")

    def feed(self, rows, borders):
        out = out_tensor(self.model, len(rows))
        lo, hi = np.ascontiguousarray(borders[:, 0], np.int32), np.ascontiguousarray(borders[:, 1], np.int32)
        _lib.check(self.lib.vp_sweep_bank(self.h, self.bank.handle, ptr(rows), ptr(lo), ptr(hi), len(rows), G._norm(self.model.norm),
                                          *E._sweep_rows(self.model), C.c_void_p(out.data_ptr())), "vp_sweep_bank")
        return out

    def end(self, n):
        NT, nw = len(self.on), C.c_longlong()
        count, peak, value = np.zeros((n, 2, NT), np.int32), np.zeros((n, 2, NT, self.K), np.int32), np.zeros((n, 2, NT, self.K), np.float32)
        _lib.check(self.lib.vp_sweep_end(self.h, ptr(count), ptr(peak), ptr(value), n, C.byref(nw)), "vp_sweep_end")
        assert nw.value == n
        return count, peak, value


class ValidationPass(PredictPass):
    def begin(self):
        self.sizes = []
        _lib.check(self.lib.vp_validate_begin(self.h), "vp_validate_begin")

    def feed(self, rows, borders=None):
        out = out_tensor(self.model, len(rows))
        name = "vp_validate_bank_aug" if rows.dtype == G.AUG_ROW else "vp_validate_bank"
        lrows = G.label_rows(self.model.labels)
        _lib.check(getattr(self.lib, name)(self.h, self.bank.handle, ptr(rows), len(rows), float(SIGMA), G._norm(self.model.norm),
                                           lrows.ctypes.data_as(C.POINTER(C.c_int)), 1e-5, C.c_void_p(out.data_ptr())), name)
        self.sizes.append(len(rows))
        return out

    def end(self, n):
        batch, window = np.empty(len(self.sizes), np.float64), np.empty(n, np.float64)
        nb, nw = C.c_longlong(), C.c_longlong()
        as_double = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(self.lib.vp_validate_end(self.h, as_double(batch), len(batch), C.byref(nb), as_double(window), n, C.byref(nw)),
                   "vp_validate_end")
        assert (nb.value, nw.value) == (len(batch), n) and sum(self.sizes) == n
        return batch, window


def run_pass(p, batches):
    """One pass over ``batches`` ((rows, borders) each) -> (the pass's result, the batches' probabilities).  The
    probabilities are written on the handle's stream: they are read once the pass has ended, which waits for it."""
    p.begin()
    preds = [p.feed(rows, borders) for rows, borders in batches]
    result = p.end(sum(len(rows) for rows, _ in batches))
    return result, [t.cpu().numpy() for t in preds]


def one_at_a_time(p, batches):
    """Every batch as a pass of its own, the results concatenated."""
    parts = [run_pass(p, [b])[0] for b in batches]
    return tuple(np.concatenate([part[i] for part in parts]) for i in range(len(parts[0])))


def cut(rows, borders, sizes, first=0):
    """Consecutive batches of ``sizes`` windows, the rows taken round and round."""
    out = []
    for B in sizes:
        ix = np.arange(first, first + B) % len(rows)
        out.append((rows[ix], None if borders is None else borders[ix]))
        first += B
    return out


def validation_batches(bank, sizes, seed, big_is_augmented=True):
    """Plain and augmented row batches in turn; a batch above max_batch is augmented (the larger row: it outgrows the slots)."""
    kinds = ["augmented" if (B > MAX_BATCH and big_is_augmented) or (B <= MAX_BATCH and i % 2) else "window" for i, B in enumerate(sizes)]
    return [(planned_rows(bank, B, kind, seed=seed + i), None) for i, (B, kind) in enumerate(zip(sizes, kinds))]


@pytest.mark.parametrize("kind", ["predict", "sweep"])
@pytest.mark.parametrize("name", ["phasenet", "eqtransformer"])
def test_a_pass_wraps_the_ring_then_regrows(name, kind):
    Pass = {"predict": PredictPass, "sweep": SweepPass}[kind]
    model, other = fresh_model(name), fresh_model(name)
    T = model.in_samples
    bank, _, targets = mixed_bank(T, seed=3)
    try:
        rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        batches = cut(rows, borders, SIZES)
        assert len(batches) == 2 * RING + 5 and max(SIZES) > MAX_BATCH
        got, preds = run_pass(Pass(model, bank), batches)
        assert same(got, one_at_a_time(Pass(other, bank), batches))
        if kind == "sweep":
            assert got[0].sum() > 0 and got[0].max() <= SweepPass.K
        y = direct(other, bank, rows)
        first = 0
        for (r, _), p in zip(batches, preds):
            assert np.array_equal(bits(p), bits(y[np.arange(first, first + len(r)) % len(rows)])), first
            first += len(r)
    finally:
        bank.close()


def test_a_validation_pass_wraps_the_ring_then_regrows():
    model, other = fresh_model("phasenet"), fresh_model("phasenet")
    _, _, _, bank = synthetic_bank(40, L=9000, seed=12)
    try:
        batches = validation_batches(bank, SIZES, seed=70)
        assert {r.dtype for r, _ in batches[:2 * RING + 3]} == {G.PLAN_ROW, G.AUG_ROW} and batches[-2][0].dtype == G.AUG_ROW
        plans = [r for r, _ in batches]
        batch, window, preds = validate_batches(model, bank, plans, SIGMA, predictions=True)
        assert batch.shape == (len(SIZES),) and window.shape == (sum(SIZES),) and np.isfinite(window).all()
        assert same((batch, window), one_at_a_time(ValidationPass(other, bank), batches))
        for r, p in zip(plans, preds):
            want = other(bank.make_batch(r, other, SIGMA)["X"]).cpu().numpy()
            assert np.array_equal(bits(p.cpu().numpy()), bits(want))
    finally:
        bank.close()


def test_three_passes_open_at_once_on_one_handle():
    """Opened validation, prediction, sweep; fed round robin, each with one batch above max_batch in another round; closed
    prediction, sweep, validation.  Each holds what it holds when it runs alone."""
    model = fresh_model("phasenet")
    T = model.in_samples
    _, _, _, vbank = synthetic_bank(40, L=9000, seed=12)
    bank, _, targets = mixed_bank(T, seed=3)
    try:
        rows, borders = G.SteeredPlanner(bank, T).plan(targets)
        fed = {"val": validation_batches(vbank, [3, 12, 2], seed=90), "prd": cut(rows, borders, [2, 3, 11]),
               "swp": cut(rows, borders, [9, 1, 4], first=16)}
        passes = {"val": ValidationPass(model, vbank), "prd": PredictPass(model, bank), "swp": SweepPass(model, bank)}
        for k in ("val", "prd", "swp"):
            passes[k].begin()
        preds = {k: [] for k in passes}
        for i in range(3):
            for k in ("val", "prd", "swp"):
                preds[k].append(passes[k].feed(*fed[k][i]))
        got = {k: passes[k].end(sum(len(r) for r, _ in fed[k])) for k in ("prd", "swp", "val")}
        preds = {k: [t.cpu().numpy() for t in v] for k, v in preds.items()}  # (every end has waited for the handle's stream)
        for k in passes:
            alone, alone_preds = run_pass(passes[k], fed[k])
            assert same(got[k], alone), k
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(preds[k], alone_preds)), k
        assert got["swp"][0].sum() > 0 and np.isfinite(got["val"][1]).all()
    finally:
        bank.close()
        vbank.close()


def test_make_batch_wraps_the_banks_ring_then_regrows():
    w, ps, ss, bank = synthetic_bank(40, L=9000, seed=12)
    model = fresh_model("phasenet")
    sizes = SIZES[:-2] + [24, 2]
    try:
        plans = [planned_rows(bank, B, "augmented" if i % 2 else "window", seed=110 + i) for i, B in enumerate(sizes)]
        assert plans[-2].dtype == G.AUG_ROW and plans[-2].nbytes > max(p.nbytes for p in plans[:-2])
        made = [bank.make_batch(r, model, SIGMA) for r in plans]
        torch.cuda.synchronize()
        for i, (r, m) in enumerate(zip(plans, made)):
            fresh = G.WaveformBank(w, {"P": ps, "S": ss})
            try:
                want = fresh.make_batch(r, model, SIGMA)
                assert all(np.array_equal(bits(m[k].cpu().numpy()), bits(want[k].cpu().numpy())) for k in ("X", "y")), i
            finally:
                fresh.close()
    finally:
        bank.close()
