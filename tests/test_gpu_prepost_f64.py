"""The two ends of every annotate() / classify() call against float64, each stage on its own input (tests/prepost_f64.py; the
bounds' teeth: tests/test_prepost_f64_cpu.py).

Preprocessing: the input tensor that gather_normalize_kernel writes, read back with debug_tensors, against ``pre64`` of the raw
windows -- dense batches of the hard inputs, and the last batch of a stream with a tail window; the in-kernel twins
(pn_window_kernel, eqt_front_kernel) bit for bit against the gather-kernel plan on the same inputs; the window table of
vp_classify_multi over blocks of unequal length, read the same way.

Stacking: per model on ONE handle, in table order, ``_annotate_block`` against ``stack64`` of the dense predictions of the
host-cut windows: n_windows / first_valid / last_valid, the NaN pattern over all N samples, max bit for bit, avg within the bound;
then three cases again on a fresh handle (nothing stale is read from the grown, never cleared buffers), and stack_multi_kernel
against vp_annotate.

Not in scope: the 64-bit instantiation stack_kernel<long> (reached only from N + T >= 2^31, about 77 GB of device buffers per
call), the trigger scan (compared exactly in tests/test_gpu_parity_gaps.py), resampling, miniSEED.

Measured on an MI355X (worst |got - want| / bound): see LOG.md, "Preprocessing and stacking against float64"."""
import ctypes as C

import numpy as np
import pytest

from oracle import pipeline as OP
from tests.gpu_util import debug_tensors
from tests.prepost_f64 import (CONFIGS, IN_SAMPLES, STACK_CASES, effective, pre64, pre_inputs, pre_ratio, stack64, stack_case_id,
                               stack_ratio, valid_range)
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows

pytestmark = pytest.mark.gpu

CLS = {"PhaseNet": PhaseNet, "EQTransformer": EQTransformer}
# plans whose input tensor holds what gather_normalize_kernel wrote when the forward pass is over (the ones the parity tests
# read `input` from), the gather-kernel plans of the bit-identity tests, and the plans with the in-kernel twins
READ_PLAN = {"PhaseNet": (0, 0, 0, 0, 0, 2), "EQTransformer": (0, 0)}
GATHER_PLAN = {"PhaseNet": (0, 0, 0, 0, 0, 0, 1), "EQTransformer": (0, 0)}
TWIN_PLAN = {"PhaseNet": (0, 0), "EQTransformer": (0, 0, 0, 0, 0, 0, 2)}
CFG_IDS = [c[0] for c in CONFIGS]


def _make(name, norm="peak", per_comp=False, flags=(0, 0)):
    m = CLS[name].from_pretrained("volpick")
    m.norm = norm
    if name == "EQTransformer":
        m.norm_amp_per_comp = bool(per_comp)
    m._plan_flags = flags
    return m.cuda()


def _stream(N, seed, offset=True):
    data, _, _ = synthetic_stream_array(N, seed=seed)
    if offset:
        data[1] += 321.0
        data[2] *= 40.0
    return data


def _cut(data, starts, T):
    if len(starts) == 0:
        return np.empty((0, 3, T), np.float32)
    return np.stack([data[:, s:s + T] for s in starts]).astype(np.float32)


def _classify_multi(m, blocks, overlap, bl, br, mode, batch=256):
    """vp_classify_multi on (3, N_k) blocks -> ([rows (3, N_k)], first_valid, last_valid, n_windows per block); call pattern of
    tests/test_gpu_async.py::test_classify_multi_rows_match_annotate_and_argument_errors."""
    lib = _lib.load()
    h = m._ensure_handle()
    I64 = C.POINTER(C.c_int64)
    cap = 4096
    on, off, pk = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int64)
    val, so, bo = np.empty(cap, np.float32), np.empty(cap, np.int32), np.empty(cap, np.int32)
    specs = (_lib.VpTriggerSpec * 2)(_lib.VpTriggerSpec(0, 0.3, 0.3), _lib.VpTriggerSpec(1, 0.3, 0.3))
    lens = np.array([b.shape[1] for b in blocks], np.int64)
    offs = np.concatenate([[0], np.cumsum(3 * lens)[:-1]]).astype(np.int64)
    flat = np.concatenate([b.reshape(-1) for b in blocks]).astype(np.float32)
    out = np.empty_like(flat)
    K = len(blocks)
    fv, lv, nw = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
    found = C.c_int()
    stk = _lib.VP_STACK_AVG if mode == "avg" else _lib.VP_STACK_MAX
    _lib.check(lib.vp_classify_multi(
        h, flat.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST, offs.ctypes.data_as(I64), lens.ctypes.data_as(I64), K,
        overlap, bl, br, stk, batch, specs, 2, out.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST,
        fv.ctypes.data_as(I64), lv.ctypes.data_as(I64), nw.ctypes.data_as(I64), on.ctypes.data_as(I64),
        off.ctypes.data_as(I64), pk.ctypes.data_as(I64), val.ctypes.data_as(C.POINTER(C.c_float)),
        so.ctypes.data_as(C.POINTER(C.c_int32)), bo.ctypes.data_as(C.POINTER(C.c_int32)), 256, cap, C.byref(found)),
        "vp_classify_multi")
    rows = [out[o:o + 3 * n].reshape(3, n) for o, n in zip(offs, lens)]
    return rows, fv, lv, nw


# ---------------------------------------------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_gather_normalize_matches_float64(cfg):
    cid, name, norm, per_comp = cfg
    T = IN_SAMPLES[name]
    m = _make(name, norm, per_comp, READ_PLAN[name])
    bad = []
    for iname, x in pre_inputs(T, seed=11, peak_only=effective(name, norm, per_comp)[0] == "peak").items():
        want, bound = pre64(x, name, norm, per_comp)
        m._forward_raw(x, preprocess=True)
        got = debug_tensors(m, len(x))["input"]
        assert got.shape == x.shape
        r = pre_ratio(got, want, bound)
        print(f"gather {cid:12s} {iname:11s} {r:8.3f} of the bound")
        if not r <= 1.0:
            bad.append((iname, r))
    m._release()
    assert not bad, (cid, bad)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_stream_windows_match_float64(cfg):
    """The stream source of the gather kernel: a batch smaller than the window count, so that the input tensor holds the
    last batch when the call returns -- windows first_window + w, the last one flush with the end of the stream."""
    cid, name, norm, per_comp = cfg
    T = IN_SAMPLES[name]
    overlap = T // 2
    N = T + 5 * (T - overlap) + 137
    data = _stream(N, seed=41)
    starts = OP.window_starts(N, T, overlap)
    assert len(starts) == 7 and starts[-1] == N - T and starts[-1] - starts[-2] == 137
    m = _make(name, norm, per_comp, READ_PLAN[name])
    args = m._argdict(dict(overlap=overlap, blinding=(0, 0), stacking="avg", batch_size=4))
    _, _, _, nw = m._annotate_block(data, args)
    assert nw == 7
    got = debug_tensors(m, 3)["input"]  # the second batch: windows 4, 5 and the tail
    want, bound = pre64(_cut(data, starts[4:], T), name, norm, per_comp)
    m._release()
    r = pre_ratio(got, want, bound)
    print(f"stream {cid:12s} {r:8.3f} of the bound")
    assert r <= 1.0, (cid, r)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_classify_multi_window_table_matches_float64(cfg):
    """The third source of the gather kernel: the window table of vp_classify_multi over blocks of unequal length -- one without
    a tail window, one of exactly T samples, one with a tail, one too short for a window.  All windows fit one batch, so the
    input tensor holds them in table order when the call returns."""
    cid, name, norm, per_comp = cfg
    T = IN_SAMPLES[name]
    overlap = T // 2
    step = T - overlap
    blocks = [_stream(n, seed=60 + i) for i, n in enumerate((T + 3 * step, T, T + step + 137, T - 1))]
    starts = [OP.window_starts(b.shape[1], T, overlap) for b in blocks]
    assert [len(s) for s in starts] == [4, 1, 3, 0]
    m = _make(name, norm, per_comp, READ_PLAN[name])
    _, fv, lv, nw = _classify_multi(m, blocks, overlap, 0, 0, "avg")
    assert list(nw) == [4, 1, 3, 0] and list(fv) == [0, 0, 0, -1]
    got = debug_tensors(m, 8)["input"]
    m._release()
    want, bound = pre64(np.concatenate([_cut(b, s, T) for b, s in zip(blocks, starts)]), name, norm, per_comp)
    r = pre_ratio(got, want, bound)
    print(f"table  {cid:12s} {r:8.3f} of the bound")
    assert r <= 1.0, (cid, r)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_in_kernel_twins_are_bitwise_the_gather_kernel_on_the_hard_inputs(cfg):
    """pn_window_kernel (PhaseNet's default plan) and eqt_front_kernel (plan_flags[6] = 2) normalise their windows themselves:
    the probabilities of the gather-kernel plan bit for bit, on the inputs where the reductions could differ, with a NaN and
    an Inf window among them, dense and from a stream with a tail window."""
    cid, name, norm, per_comp = cfg
    T = IN_SAMPLES[name]
    twin = _make(name, norm, per_comp, TWIN_PLAN[name])
    gather = _make(name, norm, per_comp, GATHER_PLAN[name])
    inputs = pre_inputs(T, seed=11, peak_only=effective(name, norm, per_comp)[0] == "peak")
    nf = synthetic_windows(6, T, seed=5)
    nf[1, 2, T - 3] = np.nan
    nf[4, 0, 1000] = np.inf
    inputs["nan+inf"] = nf
    differ = []
    for iname, x in inputs.items():
        a, b = twin._forward_raw(x, preprocess=True), gather._forward_raw(x, preprocess=True)
        if iname == "nan+inf":
            assert np.isnan(a[[1, 4]]).all() and np.isfinite(a[[0, 2, 3, 5]]).all()
        if not np.array_equal(a, b, equal_nan=True):
            differ.append((iname, int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())))
    overlap = T // 2
    data = _stream(T + 5 * (T - overlap) + 137, seed=41)
    args = twin._argdict(dict(overlap=overlap, blinding=(0, 0), stacking="avg", batch_size=4))
    a = twin._annotate_block(data, args)[0].cpu().numpy()
    b = gather._annotate_block(data, args)[0].cpu().numpy()
    if not np.array_equal(a, b, equal_nan=True):
        differ.append(("stream", int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())))
    twin._release(), gather._release()
    assert not differ, (cid, differ)


# ---------------------------------------------------------------------------------------------------------- stacking
def _case_stream(T, ci, case):
    N = case[0]
    data = _stream(N, seed=900 + ci, offset=False)
    if N >= 3 * T:
        data[1, N // 2] = np.nan  # its windows are flagged: all their predictions are NaN, and stacking skips them
    return data


def _run_case(m, T, ci, case):
    """-> (rows (3, N) ndarray, list of failures) for one case of the table on handle m."""
    N, overlap, bl, br, mode = case
    data = _case_stream(T, ci, case)
    starts = OP.window_starts(N, T, overlap)
    preds = m._forward_raw(_cut(data, starts, T), preprocess=True) if len(starts) else np.empty((0, 3, T), np.float32)
    args = m._argdict(dict(overlap=overlap, blinding=(bl, br), stacking=mode))
    out, fv, lv, nw = m._annotate_block(data, args)
    out = out.cpu().numpy()
    want, cnt, bound = stack64(preds, starts, T, N, bl, br, mode)
    fails = []
    if (nw, fv, lv) != valid_range(starts, T, bl, br):
        fails.append(("range", (nw, fv, lv), valid_range(starts, T, bl, br)))
    same, r = stack_ratio(out, want, bound)
    if not same:
        fails.append(("NaN pattern", int((np.isnan(out) != np.isnan(want)).sum())))
    if mode == "max" and not np.array_equal(out, want.astype(np.float32), equal_nan=True):
        fails.append(("max is not exact", r))
    if not r <= 1.0:
        fails.append(("bound", r))
    print(f"stack {m.name:13s} {stack_case_id(case):36s} windows {nw:5d} count <= {int(cnt.max()):4d} NaN samples "
          f"{int(np.isnan(out).sum()):6d}  {r:6.3f} of the bound")
    return out, fails


FRESH = (2, 7, 14)  # a small N behind a large one; the smaller blinding behind the larger; the call behind the empty one


@pytest.mark.parametrize("name", ["PhaseNet", "EQTransformer"])
def test_stacking_matches_float64_on_one_handle(name):
    T = IN_SAMPLES[name]
    m = _make(name)
    # first of all: without overlap and blinding the stacked rows ARE the dense predictions (count 1: 0 + v and v / 1 are exact),
    # which ties the windows of the stream path to those of the dense call; every comparison below rests on it
    data = _stream(4 * T, seed=899, offset=False)
    preds = m._forward_raw(_cut(data, np.arange(4) * T, T), preprocess=True)
    out, fv, lv, nw = m._annotate_block(data, m._argdict(dict(overlap=0, blinding=(0, 0), stacking="avg")))
    assert (nw, fv, lv) == (4, 0, 4 * T - 1)
    assert np.array_equal(out.cpu().numpy(), preds.transpose(1, 0, 2).reshape(3, 4 * T)), \
        "the stream path's predictions are not the dense call's: nothing below can be compared"
    cases = STACK_CASES(T)
    kept, fails = {}, []
    for ci, case in enumerate(cases):
        out, f = _run_case(m, T, ci, case)
        if ci in FRESH:
            kept[ci] = out
        fails += [(stack_case_id(case),) + tuple(x) for x in f]
    m._release()
    assert not fails, fails
    for ci in FRESH:  # nothing stale was read from d_pred, the input tensor or the tail kernel's unwritten blinded tiles
        fresh = _make(name)
        out, f = _run_case(fresh, T, ci, cases[ci])
        fresh._release()
        assert not f and np.array_equal(out, kept[ci], equal_nan=True), (stack_case_id(cases[ci]), f)


@pytest.mark.parametrize("name", ["PhaseNet", "EQTransformer"])
def test_classify_multi_matches_annotate_at_the_table_edges(name):
    """stack_multi_kernel and the window table of vp_classify_multi: for every (overlap, blinding, stacking) of the table, the
    table's streams go through ONE call as blocks of unequal length (among them one of exactly T samples, one shorter, one
    without a tail window), and every block's rows, first_valid, last_valid, n_windows equal its vp_annotate bit for bit.
    (A setting takes the streams that give it at most 600 windows each: step 1 on 60000 samples would be 57000.)"""
    T = IN_SAMPLES[name]
    lib = _lib.load()
    m = _make(name)
    h = m._ensure_handle()
    cases = STACK_CASES(T)
    streams = {}
    for ci, case in enumerate(cases):
        streams.setdefault(case[0], _case_stream(T, ci, case))
    differ = []
    for overlap, bl, br, mode in sorted({c[1:] for c in cases}):
        blocks = [streams[n] for n in sorted(streams) if len(OP.window_starts(n, T, overlap)) <= 600]
        assert len(blocks) >= 4
        rows, fv, lv, nw = _classify_multi(m, blocks, overlap, bl, br, mode)
        stk = _lib.VP_STACK_AVG if mode == "avg" else _lib.VP_STACK_MAX
        for k, b in enumerate(blocks):
            n = b.shape[1]
            want = np.empty((3, n), np.float32)
            f1, l1, n1 = C.c_int64(), C.c_int64(), C.c_int64()
            _lib.check(lib.vp_annotate(h, np.ascontiguousarray(b, np.float32).ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST, n,
                                       overlap, bl, br, stk, 256, want.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST,
                                       C.byref(f1), C.byref(l1), C.byref(n1)), "vp_annotate")
            got = rows[k]
            starts = OP.window_starts(n, T, overlap)
            if (fv[k], lv[k], nw[k]) != (f1.value, l1.value, n1.value) or (n1.value, f1.value, l1.value) != valid_range(starts, T, bl, br):
                differ.append(((overlap, bl, br, mode), n, "range", (int(nw[k]), int(fv[k]), int(lv[k])), (n1.value, f1.value, l1.value)))
            if not np.array_equal(got, want, equal_nan=True):
                differ.append(((overlap, bl, br, mode), n, "rows", int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())))
        print(f"multi {name:13s} overlap {overlap:5d} blinding ({bl}, {br}) {mode}: {len(blocks)} blocks, {int(nw.sum())} windows")
    m._release()
    assert not differ, differ
