"""GPU: the trigger / peak extraction on made-up traces, through every entry point that reaches it.

The traces of tests/trigger_cases.py are laid against the grid of the kernels in volpick_amd/csrc/prepost.hip (1024-sample
chunks, the 512-entry run-end list, the 256-sample walk-back trip, the lane-strided first argmax, the flat word copy of
publish_kernel, the 1/64 lane segments of window_pick_kernel); the expected answers are oracle.pipeline.picks_from_trace on the
same samples, which tests/test_trigger_cases_cpu.py holds against two more statements of the rule.  Everything is exact: indices
as integers, values bit for bit.

  vp_pick            every family, device trace
  vp_pick_rows       1 / 4 / 5 / 16 specs over three rows, per-spec counts 0, 1, 255, 256, 257, > 1000; cap below the total;
                     one handle's result block reused under three (n_specs, cap) layouts; argument errors
  vp_classify_multi, vp_classify, submit / collect
                     network rows made dense by thresholds at the rows' medians (> 256 triggers in a row), cap_per_row
                     below the count, the retry loops of Model._classify_blocks and Model._collect_block
  vp_pick_windows    9 windows (a partial workgroup), runs across the lane-segment seams, borders that cut runs, len 1 / 63 /
                     64 / 65, clipped and empty borders, K below the count, host and device `prob`, evaluate_windows' error
  64-bit positions   trigger_scan_kernel<long> on a device trace of 2^31 + 5000 samples (slow)

Not reached: trigger_scan_table_kernel<long> (one vp_classify_multi block longer than 2^31 - 4097 samples: 26 GB of input rows
and 715,000 forward windows).
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import volpick_amd as va
from oracle import pipeline as OP
from tests import trigger_cases as TC
from volpick_amd import _lib
from volpick_amd.evaluate import evaluate_windows

pytestmark = pytest.mark.gpu

I64, I32, F32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
DEV, HOST = _lib.VP_MEM_DEVICE, _lib.VP_MEM_HOST


@pytest.fixture(scope="module")
def pn():
    return va.PhaseNet.from_pretrained("volpick").cuda()


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------------- vp_pick
def _pick_dev(h, d, n, thr_on, thr_off, cap):
    """vp_pick on `n` floats of the device tensor `d` -> ([(on, off, peak, value)], n_found)."""
    lib = _lib.load()
    on, off, pk = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int64)
    val, found = np.empty(cap, np.float32), C.c_int()
    _lib.check(lib.vp_pick(h, C.c_void_p(d.data_ptr()), DEV, n, thr_on, thr_off, on.ctypes.data_as(I64),
                           off.ctypes.data_as(I64), pk.ctypes.data_as(I64), val.ctypes.data_as(F32), cap, C.byref(found)),
               "vp_pick")
    m = min(found.value, cap)
    return [(int(on[i]), int(off[i]), int(pk[i]), float(val[i])) for i in range(m)], found.value


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if tuple(g[:3]) != tuple(w[:3]) or np.float32(g[3]) != np.float32(w[3]):
            return f"trigger {i}: got {g}, want {w}"
    return f"{len(got)} triggers, want {len(want)}"


def test_vp_pick_every_family(pn):
    want = TC.expected()
    bad, n_trig = [], 0
    for c in TC.all_cases():
        d = torch.from_numpy(c.x.copy()).cuda()
        torch.cuda.synchronize()
        for p in c.pairs:
            w = want[(c.name, p)]
            got, n = _pick_dev(pn._handle, d, len(c.x), p[0], p[1], cap=len(c.x) // 2 + 2)
            n_trig += len(w)
            try:
                assert n == len(w), (n, len(w))
                TC.same(got, w)
            except AssertionError:
                bad.append((c.name, p, f"n_found {n}", _first_difference(got, w)))
    print(f"{len(TC.all_cases())} cases, {n_trig} triggers, {len(bad)} wrong")
    assert not bad, bad[:20]


# -------------------------------------------------------------------------------------------------------- vp_pick_rows
@lru_cache(maxsize=None)
def _three_rows():
    """(3, N) rows of three families, 16 specs [(row, thr_on, thr_off)] and every spec's expected list."""
    r0 = TC.case("alt_even").x                                 # 1540 one-sample runs
    parts = []                                                 # 257 runs: 255 at 0.9, one at 0.7, one at 0.6
    for i in range(257):
        L = (1, 2, 63, 64, 65)[i % 5]
        run = {100: 0.7, 200: 0.6}.get(i, TC.RUN)
        seg = TC.fill_run(TC.base(L + 3), 0, L, TC.FILLINGS[i % 3] if run == TC.RUN else "flat", run=run)
        parts.append(seg)
    r1 = np.concatenate(parts)
    r2 = np.concatenate([TC.case(n).x for n in ("tie_d63_gap256", "run_L1025_e2304_first", "tie_all_offsets", "nan_splits")])
    r2[40] = 0.99                                              # the one sample above 0.95
    N = max(len(r0), len(r1), len(r2)) + 13
    rows = np.full((3, N), TC.BASE, np.float32)
    for i, r in enumerate((r0, r1, r2)):
        rows[i, :len(r)] = r
    specs = [(0, .5, .5), (1, .8, .8), (2, .95, .95), (0, .95, .95), (1, .65, .65), (1, .55, .55), (0, .5, .25), (2, .5, .25),
             (2, .5, .5), (1, .8, .25), (0, .5, .01), (1, .65, .25), (2, .75, .6), (1, .55, .55), (0, .9, .9), (2, .25, .25)]
    specs = [(r, _f32(a), _f32(b)) for r, a, b in specs]
    want = [OP.picks_from_trace(rows[r], a, b) for r, a, b in specs]
    rows.setflags(write=False)
    return rows, specs, want


def _rows_call(h, dev, specs, cap):
    """vp_pick_rows -> (return code, [(spec, on, off, peak, value)] as written, n_found)."""
    lib = _lib.load()
    cs = (_lib.VpTriggerSpec * max(1, len(specs)))(*[_lib.VpTriggerSpec(r, a, b) for r, a, b in specs])
    c = max(cap, 1)
    on, off, pk = np.full(c, -7, np.int64), np.full(c, -7, np.int64), np.full(c, -7, np.int64)
    val, so, found = np.full(c, -7, np.float32), np.full(c, -7, np.int32), C.c_int(-1)
    rc = lib.vp_pick_rows(h, C.c_void_p(dev.data_ptr()), dev.shape[1], cs, len(specs), on.ctypes.data_as(I64),
                          off.ctypes.data_as(I64), pk.ctypes.data_as(I64), val.ctypes.data_as(F32), so.ctypes.data_as(I32), cap,
                          C.byref(found))
    m = max(0, min(found.value, cap))
    return rc, [(int(so[i]), int(on[i]), int(off[i]), int(pk[i]), float(val[i])) for i in range(m)], found.value


def _check_rows(got, n_found, want, cap):
    """The contract of vp_pick_rows: n_found is the true total whatever `cap`; the groups come in spec order, each sorted by
    onset; a spec whose count fits `cap` is handed out exactly (as much of it as the caller's arrays still hold), one that
    does not is handed out as `cap` of its triggers, whichever the device appended first."""
    assert n_found == sum(len(w) for w in want), (n_found, [len(w) for w in want])
    at = 0
    for i, w in enumerate(want):
        room = cap - at
        m = min(len(w), cap, room)
        grp = got[at:at + m]
        assert [g[0] for g in grp] == [i] * m, (i, [g[0] for g in grp][:8])
        if len(w) <= cap:
            TC.same([g[1:] for g in grp], w[:m])
        else:
            by_on = {t[0]: t for t in w}
            ons = [g[1] for g in grp]
            assert ons == sorted(set(ons)), i
            for g in grp:
                assert g[1] in by_on, (i, g)
                TC.same([g[1:]], [by_on[g[1]]])
        at += m
    assert at == len(got) == min(n_found, cap)


@pytest.fixture(scope="module")
def three_rows_dev():
    rows, _, _ = _three_rows()
    d = torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    return d


def test_three_rows_hold_the_counts_the_issue_names():
    _, specs, want = _three_rows()
    counts = [len(w) for w in want]
    assert len(specs) == 16 and {0, 1, 255, 256, 257} <= set(counts) and max(counts) > 1000, counts
    assert {0, 1, 255, 256} <= set(counts[:5]) and counts[0] > 1000  # the five-spec call sees them too


@pytest.mark.parametrize("n_specs", [1, 4, 5, 16])
def test_vp_pick_rows_exact(pn, three_rows_dev, n_specs):
    _, specs, want = _three_rows()
    specs, want = specs[:n_specs], want[:n_specs]
    total = sum(len(w) for w in want)
    rc, got, n = _rows_call(pn._handle, three_rows_dev, specs, cap=total + 9)
    assert rc == 0 and n == total == len(got)
    _check_rows(got, n, want, total + 9)
    flat = [(i,) + tuple(t) for i, w in enumerate(want) for t in w]
    assert [g[:4] for g in got] == [f[:4] for f in flat]  # spec_of, and every group whole and sorted by onset
    for cap in (1, 300):
        rc, got, n = _rows_call(pn._handle, three_rows_dev, specs, cap=cap)
        assert rc == 0
        _check_rows(got, n, want, cap)
        # the retry loop of the Python layer ends in the full list
        full = pn._pick_rows(three_rows_dev, [(r, "x", a, b) for r, a, b in specs], cap=cap)
        assert len(full) == total
        assert [f[:4] for f in full] == [f[:4] for f in flat]
        assert [np.float32(f[4]) for f in full] == [np.float32(f[4]) for f in flat]


def test_vp_pick_rows_result_block_reused_under_other_layouts(three_rows_dev):
    """One handle, three calls: (16 specs, large cap), (2 specs, small cap), (5 specs, middle cap).  The counters must have been
    re-armed by the call before, and no word of an earlier layout may show."""
    _, specs, want = _three_rows()
    m = va.PhaseNet.from_pretrained("volpick").cuda()
    total = sum(len(w) for w in want)
    rc, got, n = _rows_call(m._handle, three_rows_dev, specs, cap=total + 100)
    assert rc == 0
    _check_rows(got, n, want, total + 100)
    pick = [5, 0]                    # 257 and 1540 triggers into room for 3
    rc, got, n = _rows_call(m._handle, three_rows_dev, [specs[i] for i in pick], cap=3)
    assert rc == 0
    _check_rows(got, n, [want[i] for i in pick], 3)
    pick = [1, 2, 3, 4, 0]           # 255 + 1 + 0 + 256 whole, then what is left of 600 from a spec of 1540
    rc, got, n = _rows_call(m._handle, three_rows_dev, [specs[i] for i in pick], cap=600)
    assert rc == 0 and len(got) == 600
    _check_rows(got, n, [want[i] for i in pick], 600)
    rc, got, n = _rows_call(m._handle, three_rows_dev, specs, cap=total)  # and the first layout again, exactly full
    assert rc == 0 and len(got) == total
    _check_rows(got, n, want, total)
    m._release()


def test_vp_pick_rows_argument_errors(pn, three_rows_dev):
    _, specs, _ = _three_rows()
    h = pn._handle
    lib = _lib.load()
    assert _rows_call(h, three_rows_dev, [(0, _f32(.25), _f32(.5))], 8)[0] < 0 and b"thr_off" in lib.vp_last_error()
    assert _rows_call(h, three_rows_dev, [(3, .5, .5)], 8)[0] < 0 and b"row 3" in lib.vp_last_error()
    assert _rows_call(h, three_rows_dev, [(-1, .5, .5)], 8)[0] < 0
    assert _rows_call(h, three_rows_dev, [], 8)[0] < 0
    assert _rows_call(h, three_rows_dev, specs + specs[:1], 8)[0] < 0
    assert _rows_call(h, three_rows_dev, specs[:1], -1)[0] < 0
    rc, got, n = _rows_call(h, three_rows_dev, specs[:1], 0)  # count only
    assert rc == 0 and got == [] and n == 1540


# -------------------------------------------------------------------------------- vp_classify_multi, vp_classify, submit
T_PN, OVERLAP, BLIND, BATCH = 3001, 1500, (100, 200), 64
BLOCK_LENGTHS = (T_PN + 1500 * 29 + 517, 2000, 4099, 6007)  # 31 windows; shorter than a window; none a multiple of 1024


@lru_cache(maxsize=None)
def _noise_blocks():
    """White noise: the network's rows wiggle about their medians, one crossing per hundred samples or so."""
    rng = np.random.default_rng(77)
    return [np.ascontiguousarray(rng.standard_normal((3, n)) * (1.0 + k), np.float32) for k, n in enumerate(BLOCK_LENGTHS)]


def _multi(h, blocks, specs, cap_per_row, cap):
    """vp_classify_multi, host blocks in, host rows out -> (rows per block, {(block, spec): [(on, off, peak, value)]},
    n_found, first_valid, last_valid, n_windows)."""
    lib = _lib.load()
    lens = np.array([b.shape[1] for b in blocks], np.int64)
    offs = np.concatenate([[0], np.cumsum(3 * lens)[:-1]]).astype(np.int64)
    flat = np.concatenate([b.reshape(-1) for b in blocks]).astype(np.float32)
    out = np.empty_like(flat)
    K = len(blocks)
    fv, lv, nw = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
    on, off, pk = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int64)
    val, so, bo, found = np.empty(cap, np.float32), np.empty(cap, np.int32), np.empty(cap, np.int32), C.c_int()
    cs = (_lib.VpTriggerSpec * len(specs))(*[_lib.VpTriggerSpec(r, a, b) for r, a, b in specs])
    _lib.check(lib.vp_classify_multi(
        h, flat.ctypes.data_as(C.c_void_p), HOST, offs.ctypes.data_as(I64), lens.ctypes.data_as(I64), K, OVERLAP, BLIND[0],
        BLIND[1], _lib.VP_STACK_AVG, BATCH, cs, len(specs), out.ctypes.data_as(C.c_void_p), HOST, fv.ctypes.data_as(I64),
        lv.ctypes.data_as(I64), nw.ctypes.data_as(I64), on.ctypes.data_as(I64), off.ctypes.data_as(I64), pk.ctypes.data_as(I64),
        val.ctypes.data_as(F32), so.ctypes.data_as(I32), bo.ctypes.data_as(I32), cap_per_row, cap, C.byref(found)),
        "vp_classify_multi")
    rows = [out[o:o + 3 * n].reshape(3, n) for o, n in zip(offs, lens)]
    if found.value > cap:  # some row overflowed its list (or the caller's arrays): only the count means anything
        return rows, None, found.value, fv, lv, nw
    trig = {(k, i): [] for k in range(K) for i in range(len(specs))}
    order = []
    for j in range(found.value):
        trig[(int(bo[j]), int(so[j]))].append((int(on[j]), int(off[j]), int(pk[j]), float(val[j])))
        order.append((int(bo[j]), int(so[j])))
    assert order == sorted(order)  # block by block, spec by spec
    return rows, trig, found.value, fv, lv, nw


def _median_specs(rows):
    """Two specs per row at the median of the row over all blocks: (thr, thr) and (thr, thr / 2)."""
    allr = np.concatenate(rows, axis=1)
    specs = []
    for r in range(3):
        thr = _f32(np.nanmedian(allr[r]))
        assert 0.0 < thr < 1.0
        specs += [(r, thr, thr), (r, thr, _f32(thr / 2))]
    return specs


def test_classify_multi_and_classify_on_dense_rows(pn):
    h = pn._handle
    blocks = _noise_blocks()
    K = len(blocks)
    # thresholds nothing reaches: no trigger; the rows come back
    rows, trig, n, fv, lv, nw = _multi(h, blocks, [(r, 2.0, 2.0) for r in range(3)], cap_per_row=64, cap=1024)
    assert n == 0 and all(t == [] for t in trig.values())
    assert nw.tolist() == [len(OP.window_starts(L, T_PN, OVERLAP)) for L in BLOCK_LENGTHS] and nw[0] >= 3 and nw[1] == 0
    assert np.isnan(rows[1]).all() and np.isnan(rows[0][:, :BLIND[0]]).all() and np.isnan(rows[0][:, -BLIND[1]:]).all()
    specs = _median_specs(rows)
    # dense: every (block, spec) list against the rule on the rows THIS call returned
    rows2, trig, n, *_ = _multi(h, blocks, specs, cap_per_row=8192, cap=K * len(specs) * 8192)
    want = {(k, i): OP.picks_from_trace(rows2[k][r], a, b) for k in range(K) for i, (r, a, b) in enumerate(specs)}
    counts = {key: len(w) for key, w in want.items()}
    print("triggers per (block, spec):", counts)
    assert max(counts.values()) > 256, counts  # a row past one pass of publish_table_kernel's 256 threads
    assert n == sum(counts.values())
    for key in want:
        TC.same(trig[key], want[key])
    for a, b in zip(rows, rows2):
        assert np.array_equal(a, b, equal_nan=True)
    # a row list too short: reported, not silently cut
    cap = K * len(specs) * 256
    _, _, n, *_ = _multi(h, blocks, specs, cap_per_row=256, cap=cap)
    assert n > cap
    # the retry loop of the Python layer, from one slot per row up
    args = pn._argdict(dict(overlap=OVERLAP, blinding=BLIND, stacking="avg", batch_size=BATCH))
    pspecs = [(r, "x", a, b) for r, a, b in specs]
    lists = pn._classify_blocks([{"data": b} for b in blocks], args, pspecs, cap_per_row=1)
    for k in range(K):
        flat = [(i,) + tuple(t) for i in range(len(specs)) for t in want[(k, i)]]
        assert [g[:4] for g in lists[k]] == [f[:4] for f in flat], k
        assert [np.float32(g[4]) for g in lists[k]] == [np.float32(f[4]) for f in flat]

    # vp_classify on the long block alone: its own rows, its own lists
    lib = _lib.load()
    x = blocks[0]
    N = x.shape[1]
    out = np.empty((3, N), np.float32)
    cap = 16384
    on, off, pk = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int64)
    val, so, found = np.empty(cap, np.float32), np.empty(cap, np.int32), C.c_int()
    f1, l1, n1 = C.c_int64(), C.c_int64(), C.c_int64()
    cs = (_lib.VpTriggerSpec * len(specs))(*[_lib.VpTriggerSpec(r, a, b) for r, a, b in specs])
    _lib.check(lib.vp_classify(h, x.ctypes.data_as(C.c_void_p), HOST, N, OVERLAP, BLIND[0], BLIND[1], _lib.VP_STACK_AVG, BATCH,
                               cs, len(specs), out.ctypes.data_as(C.c_void_p), HOST, C.byref(f1), C.byref(l1), C.byref(n1),
                               on.ctypes.data_as(I64), off.ctypes.data_as(I64), pk.ctypes.data_as(I64), val.ctypes.data_as(F32),
                               so.ctypes.data_as(I32), cap, C.byref(found)), "vp_classify")
    want1 = [OP.picks_from_trace(out[r], a, b) for r, a, b in specs]
    flat = [(i,) + tuple(t) for i, w in enumerate(want1) for t in w]
    assert found.value == len(flat) > 256 and (f1.value, l1.value, n1.value) == (BLIND[0], N - BLIND[1] - 1, nw[0])
    got = [(int(so[j]), int(on[j]), int(off[j]), int(pk[j]), float(val[j])) for j in range(found.value)]
    assert [g[:4] for g in got] == [f[:4] for f in flat]
    assert [np.float32(g[4]) for g in got] == [np.float32(f[4]) for f in flat]
    # submit / collect with a result block below the count: _collect_block submits again with room
    again, nwin = pn._classify_block(x, args, pspecs, cap=8)
    assert nwin == nw[0]
    assert [tuple(int(v) for v in g[:4]) for g in again] == [f[:4] for f in flat]
    assert [np.float32(g[4]) for g in again] == [np.float32(f[4]) for f in flat]


# ------------------------------------------------------------------------------------------------------ vp_pick_windows
B_WIN, SEG = 9, -(-T_PN // 64)  # 47 samples per lane when the whole window is scanned


@lru_cache(maxsize=None)
def _window_batch():
    """(9, 3, 3001): windows cut from the families; rows differ by filling where the family has fillings."""
    T = T_PN
    p = np.full((B_WIN, 3, T), TC.BASE, np.float32)
    p[0, 0], p[0, 1], p[0, 2] = TC.case("alt_even").x[:T], TC.case("alt_odd").x[:T], TC.case("alt_even_mid").x[:T]
    for r, f in enumerate(TC.FILLINGS):
        # runs that START on the last sample of a lane segment and cross the seam (or stop just short of it)
        for j, L in enumerate((1, 2, 46, 47, 48, 63, 64, 65, 94, 95)):
            TC.fill_run(p[1, r], SEG * (4 + 6 * j) - 1, L, f)
        # runs that fill whole lane segments exactly, and one that ends on a segment's first sample
        for j, L in enumerate((SEG, 2 * SEG, SEG + 1, 3 * SEG)):
            TC.fill_run(p[2, r], SEG * (3 + 8 * j), L, f)
        at = 50
        for L in (255, 256, 257, 511, 1025):
            TC.fill_run(p[3, r], at, L, f)
            at += L + 40
        TC.fill_run(p[6, r], 0, 70, f)          # a run at sample 0
        TC.fill_run(p[6, r], T - 130, 130, f)   # a run open at the last sample
    for r, name in enumerate(("tie_d63_gap256", "tie_d0_gap64", "tie_all_offsets")):
        p[4, r, :TC.N - 700] = TC.case(name).x[700:]   # the run starts at 224
    for r, name in enumerate(("plus_inf_in_run", "nan_splits", "minus_inf_splits")):
        p[5, r, :TC.N - 500] = TC.case(name).x[500:]
    rng = np.random.default_rng(5)
    for r in range(3):
        p[7, r] = TC.random_walk(rng, T, nan=(r == 2))
    p[8, 1] = TC.RUN                             # one run, the whole window
    TC.fill_run(p[8, 2], 0, T, "last")
    p.setflags(write=False)
    return p


BORDERS = {
    "none": None,
    # a run reaches in across lo / is open at hi - 1 (windows 0, 3, 4, 6); len 64, 63, 65, 1; clipped; empty
    "a": [(1, 3000), (-5, T_PN + 10), (SEG, SEG + 64), (100, 163), (300, 365), (523, 524), (5, T_PN - 5), (200, 200), (300, 100)],
    "b": [(1000, 1063), (46, 2000), (-100, 64), (304, 563), (287, 544), (0, T_PN), (0, 1), (1500, 1565), (T_PN - 1, T_PN + 1)],
}


def _windows_call(h, prob, mem, row, borders, thr_on, thr_off, K, B=B_WIN, n_rows=3):
    lib = _lib.load()
    lo = hi = None
    if borders is not None:
        lo = np.ascontiguousarray([b[0] for b in borders], np.int32)
        hi = np.ascontiguousarray([b[1] for b in borders], np.int32)
    count = np.full(max(B, 1), -7, np.int32)
    peak = np.full((max(B, 1), max(K, 1)), -7, np.int32)
    value = np.full((max(B, 1), max(K, 1)), -7, np.float32)
    ptr = C.c_void_p(prob.data_ptr()) if mem == DEV else prob.ctypes.data_as(C.c_void_p)
    rc = lib.vp_pick_windows(h, ptr, mem, B, n_rows, row, None if lo is None else lo.ctypes.data_as(C.c_void_p),
                             None if hi is None else hi.ctypes.data_as(C.c_void_p), thr_on, thr_off, K,
                             count.ctypes.data_as(C.c_void_p), peak.ctypes.data_as(C.c_void_p),
                             value.ctypes.data_as(C.c_void_p))
    return rc, count, peak, value


def _window_want(prob, row, borders, thr_on, thr_off):
    T = prob.shape[2]
    out = []
    for b in range(prob.shape[0]):
        lo, hi = (0, T) if borders is None else borders[b]
        lo, hi = max(lo, 0), min(hi, T)
        out.append([(w[2], w[3]) for w in OP.picks_from_trace(prob[b, row, lo:hi], thr_on, thr_off)] if hi > lo else [])
    return out


def _check_windows(count, peak, value, want, K):
    for b, w in enumerate(want):
        assert count[b] == len(w), (b, int(count[b]), len(w))
        k = min(len(w), K)
        got = sorted(zip(peak[b, :k].tolist(), value[b, :k].tolist()))
        if len(w) <= K:
            assert [g[0] for g in got] == [x[0] for x in w], (b, got[:6], w[:6])
            assert [np.float32(g[1]) for g in got] == [np.float32(x[1]) for x in w], b
        else:  # any K of them, each one a trigger of the window, none twice
            by_peak = {x[0]: np.float32(x[1]) for x in w}
            assert len({g[0] for g in got}) == k and all(by_peak.get(g[0]) == np.float32(g[1]) for g in got), b


@pytest.mark.parametrize("border_set", list(BORDERS))
def test_vp_pick_windows_exact(pn, border_set):
    prob = _window_batch()
    borders = BORDERS[border_set]
    dev = torch.from_numpy(prob.copy()).cuda()
    torch.cuda.synchronize()
    K = 1600
    n_trig = 0
    for row in range(3):
        for thr_on, thr_off in TC.PAIRS:
            want = _window_want(prob, row, borders, thr_on, thr_off)
            n_trig += sum(len(w) for w in want)
            rc, count, peak, value = _windows_call(pn._handle, dev, DEV, row, borders, thr_on, thr_off, K)
            assert rc == 0
            _check_windows(count, peak, value, want, K)
            rc, count_h, peak_h, value_h = _windows_call(pn._handle, prob, HOST, row, borders, thr_on, thr_off, K)
            assert rc == 0 and np.array_equal(count, count_h)
            _check_windows(count_h, peak_h, value_h, want, K)
    assert n_trig > 100
    for name in ("a", "b"):
        lens = [min(h, T_PN) - max(l, 0) for l, h in BORDERS[name]]
        assert {1, 63, 64, 65} <= set(lens) and any(l < 0 for l, _ in BORDERS[name]) and any(h > T_PN for _, h in BORDERS[name])
    assert sorted(h - l for l, h in BORDERS["a"])[:2] == [-200, 0]  # hi < lo and hi == lo


def test_vp_pick_windows_small_k_partial_batches_and_argument_errors(pn, monkeypatch):
    prob = _window_batch()
    dev = torch.from_numpy(prob.copy()).cuda()
    torch.cuda.synchronize()
    h = pn._handle
    lib = _lib.load()
    # K below a window's count: the count is still the true number
    for K in (1, 4):
        want = _window_want(prob, 0, None, 0.5, 0.25)
        rc, count, peak, value = _windows_call(h, dev, DEV, 0, None, 0.5, 0.25, K)
        assert rc == 0 and count[0] == 1501 > K
        _check_windows(count, peak, value, want, K)
    # batches of 1 .. 8 windows: the last workgroup holds 1, 2, 3 or 4
    for B in (1, 2, 3, 4, 5, 8):
        want = _window_want(prob[:B], 1, BORDERS["a"][:B], 0.5, 0.25)
        rc, count, peak, value = _windows_call(h, dev, DEV, 1, BORDERS["a"][:B], 0.5, 0.25, 1600, B=B)
        assert rc == 0
        _check_windows(count[:B], peak[:B], value[:B], want, 1600)
    # argument errors
    for kw in (dict(B=0), dict(K=0), dict(row=3), dict(row=-1), dict(n_rows=0)):
        a = dict(row=0, K=8, B=B_WIN, n_rows=3)
        a.update(kw)
        rc, *_ = _windows_call(h, dev, DEV, a["row"], None, 0.5, 0.25, a["K"], B=a["B"], n_rows=a["n_rows"])
        assert rc < 0 and b"bad shape" in lib.vp_last_error(), kw
    rc, *_ = _windows_call(h, dev, DEV, 0, None, 0.25, 0.5, 8)
    assert rc < 0 and b"thr_off" in lib.vp_last_error()
    # evaluate_windows on an alternating window: more triggers than max_picks is an error, not a silent cut
    alt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(TC.case("alt_even").x[:T_PN], (2, 3, T_PN)))).cuda()
    monkeypatch.setattr(pn, "_forward_raw", lambda xb, **kw: alt)
    X = np.zeros((2, 3, T_PN), np.float32)
    with pytest.raises(RuntimeError, match="raise max_picks"):
        evaluate_windows(pn, X, None, threshold=0.5, max_picks=64)
    with pytest.raises(RuntimeError, match="raise max_picks"):
        evaluate_windows(pn, X, None, threshold=0.5, max_picks=1500)
    res = evaluate_windows(pn, X, None, threshold=0.5, max_picks=1501)
    assert all(r[i].tolist() == list(range(0, T_PN, 2)) for r in (res[0], res[2]) for i in range(2))
    assert all((r[i] == np.float32(TC.RUN)).all() for r in (res[1], res[3]) for i in range(2))


# ------------------------------------------------------------------------------------------------------ 64-bit positions
@pytest.mark.slow
def test_vp_pick_beyond_two_to_the_31(pn):
    """trigger_scan_kernel<long>: rows longer than 2^31 - 1 - 4096 samples are scanned with 64-bit positions.  The trace lives
    on the device only (8.6 GB); the expected list is known by construction."""
    n = 2**31 + 5000
    try:
        x = torch.full((n,), TC.BASE, dtype=torch.float32, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for a device trace of 2^31 + 5000 floats (8.6 GB)")
    m = 2**31
    x[0:10] = TC.RUN                      # at sample 0
    x[m - 3:m + 4] = TC.RUN               # across 2^31 - 1 | 2^31
    s = m + 1000
    x[s:s + 600] = TC.LOW                 # equal maxima 256 apart, beyond 2^31
    x[s + 10] = 0.8
    x[s + 266] = 0.8
    x[n - 700:n] = TC.MID                 # 700 samples to the last one, only the first above thr_on
    x[n - 700] = TC.RUN
    torch.cuda.synchronize()
    want = [(0, 9, 0, TC.RUN), (m - 3, m + 3, m - 3, TC.RUN), (s, s + 599, s + 10, 0.8), (n - 700, n - 1, n - 700, TC.RUN)]
    got, found = _pick_dev(pn._handle, x, n, 0.5, 0.25, cap=16)
    assert found == len(want)
    TC.same(got, want)
    want[3] = (n - 700, n - 700, n - 700, TC.RUN)   # thr_off = thr_on: that run is one sample long
    got, found = _pick_dev(pn._handle, x, n, 0.5, 0.5, cap=16)
    assert found == len(want)
    TC.same(got, want)
    del x
    torch.cuda.empty_cache()
