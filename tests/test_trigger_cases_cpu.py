"""CPU: the expected answers of tests/trigger_cases.py do not rest on one implementation.

For every case and threshold pair three independent statements of the rule must agree exactly: oracle.pipeline.picks_from_trace
(the ObsPy ``trigger_onset`` restatement, the reference of the GPU tests), the rule as DESIGN.md words it, written out below, and
vp_pick_host (the C++ state machine of prepost.hip) through the C ABI.  The families' own claims (counts, the 512 run ends of a
chunk, the onset in the last block of the last trip) are asserted too, so that a later edit cannot quietly empty a case.
"""
import ctypes as C

import numpy as np

from tests import trigger_cases as TC


def simple_rule(x, thr_on, thr_off):
    """Maximal runs of x > thr_off that hold a sample > thr_on; on = the first such sample, off = the run's last sample,
    peak = the first argmax over [on, off]."""
    x = np.asarray(x, np.float32)
    out, t, n = [], 0, len(x)
    while t < n:
        if not x[t] > np.float32(thr_off):
            t += 1
            continue
        e = t
        while e + 1 < n and x[e + 1] > np.float32(thr_off):
            e += 1
        hot = [s for s in range(t, e + 1) if x[s] > np.float32(thr_on)]
        if hot:
            on = hot[0]
            pk = max(range(on, e + 1), key=lambda s: (x[s], -s))
            out.append((on, e, pk, float(x[pk])))
        t = e + 1
    return out


def _pick_host(lib, x, thr_on, thr_off):
    cap = len(x) // 2 + 2
    on, off, pk = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int64)
    val, n = np.empty(cap, np.float32), C.c_int()
    I64 = C.POINTER(C.c_int64)
    assert lib.vp_pick_host(x.ctypes.data_as(C.c_void_p), len(x), thr_on, thr_off, on.ctypes.data_as(I64),
                            off.ctypes.data_as(I64), pk.ctypes.data_as(I64), val.ctypes.data_as(C.POINTER(C.c_float)), cap,
                            C.byref(n)) == 0
    assert n.value <= cap
    return [(int(on[i]), int(off[i]), int(pk[i]), float(val[i])) for i in range(n.value)]


def test_three_statements_of_the_rule_agree(lib):
    want = TC.expected()
    n_cases = n_trig = 0
    for c in TC.all_cases():
        for p in c.pairs:
            w = want[(c.name, p)]
            TC.same(simple_rule(c.x, *p), w)
            TC.same(_pick_host(lib, c.x, *p), w)
            n_trig += len(w)
        n_cases += 1
    print(f"{n_cases} cases, {n_trig} triggers")
    assert n_cases > 300 and n_trig > 7000


def test_families_hold_what_they_claim():
    want = TC.expected()
    CH, N = TC.CH, TC.N
    # alternating: every other sample ends a run, CH / 2 ends in each full chunk -- the capacity of the kernel's LDS list
    for name, count in (("alt_even", 1540), ("alt_odd", 1539)):
        x = TC.case(name).x
        for p in TC.PAIRS:
            w = want[(name, p)]
            assert len(w) == count and all(a == b == c for a, b, c, _ in w)
            for k in range(3):
                assert TC.run_ends(x, p[1], k * CH, (k + 1) * CH) == CH // 2 == 512
    assert len(want[("alt_even_mid", (0.5, 0.5))]) == 1540
    (on, off, pk, v), = want[("alt_even_mid", (0.5, 0.25))]  # ONE run of the whole trace
    assert (on, off, pk) == (0, N - 1, 0) and np.float32(v) == np.float32(TC.RUN)
    # first-only: under (0.5, 0.25) the onset is the run's first sample, found in the last block of the last trip;
    # under (0.5, 0.5) the run is one sample long
    for L in TC.LENGTHS:
        for e in TC.ENDS:
            s = e - L + 1
            if s < 0:
                continue
            (on, off, pk, _), = want[(f"run_L{L}_e{e}_first", (0.5, 0.25))]
            assert (on, off, pk) == (s, e, s)
            (on, off, pk, _), = want[(f"run_L{L}_e{e}_first", (0.5, 0.5))]
            assert (on, off, pk) == (s, s, s)
            (on, off, pk, _), = want[(f"run_L{L}_e{e}_last", (0.5, 0.25))]
            assert (on, off, pk) == (e, e, e)  # the run is L long, the trigger opens at its last sample
            (on, off, pk, _), = want[(f"run_L{L}_e{e}_flat", (0.5, 0.5))]
            assert (on, off, pk) == (s, e, s)
    # ties: the first of the equal maxima
    s = CH - 100
    for d in TC.TIE_OFFSETS:
        for gap in TC.TIE_GAPS:
            for p in TC.PAIRS:
                (on, off, pk, v), = want[(f"tie_d{d}_gap{gap}", p)]
                assert (on, off, pk) == (s, s + 599, s + d) and np.float32(v) == np.float32(0.8)
    assert want[("tie_last_only", (0.5, 0.5))][0][2] == s + 599 and want[("tie_plateau", (0.5, 0.5))][0][2] == s
    # values
    assert want[("equal_thr_on", (0.5, 0.25))] == [] and want[("equal_thr_on", (0.5, 0.5))] == []
    assert [w[:2] for w in want[("equal_thr_off", (0.5, 0.25))]] == [(CH - 20, CH - 1), (CH + 1, CH + 29)]
    (on, off, pk, v), = want[("plus_inf_in_run", (0.5, 0.5))]
    assert pk == CH + 7 and v == np.inf
    assert len(want[("minus_inf_splits", (0.5, 0.25))]) == 2 and len(want[("nan_splits", (0.5, 0.25))]) == 2
    assert want[("nan_first_sample", (0.5, 0.5))][0][:2] == (1, 29) and want[("nan_last_sample", (0.5, 0.5))][0][:2] == (N - 30, N - 2)
    assert want[("all_nan", (0.5, 0.5))] == []
    assert [w[:3] for w in want[("negative_thresholds", (-1.0, -1.25))]] == [(CH - 300, CH + 299, CH - 300),
                                                                           (2 * CH + 250, 2 * CH + 259, 2 * CH + 250)]
    assert len(want[("negative_thresholds", (-1.0, -1.0))]) == 2
    assert {len(TC.case(f"walk_n{n}_0").x) for n in TC.RANDOM_SIZES} == set(TC.RANDOM_SIZES)
