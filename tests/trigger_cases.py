"""Made-up traces for the trigger / peak extraction, shared by tests/test_trigger_cases_cpu.py and tests/test_gpu_triggers.py
(and the walk-back lengths of tests/test_gpu_parity_gaps.py::test_device_trigger_scan_edge_cases).

The families are laid against the grid of trigger_scan_kernel (volpick_amd/csrc/prepost.hip): CH samples per workgroup, whose
256 threads take 4 samples each at stride 256 and list the run ENDS of the chunk in LDS (at most CH / 2 of them); one wavefront
per run walks it back TRIP samples per trip (four 64-sample blocks) and takes the first argmax in strides of TRIP, 64 lanes by
four loads, then a wave reduction.  Everything is exact: indices are integers, a value is a sample of the trace.

Plain numpy float32; nothing here touches a GPU.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

CH = 1024    # SCAN_CHUNK: samples per workgroup
TRIP = 256   # samples per walk-back trip and per argmax stride
BASE, RUN, MID, LOW = 0.05, 0.9, 0.3, 0.7  # MID lies between the two thr_off values of PAIRS, LOW above thr_on
PAIRS = ((0.5, 0.5), (0.5, 0.25))          # (thr_on, thr_off): the picks' pair and the detections' / evaluation's pair
N = 3 * CH + 7

LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
ENDS = (CH - 1, CH, CH + 1, 2 * CH + 255, 2 * CH + 256)
FILLINGS = ("flat", "first", "last")
TIE_OFFSETS = (0, 63, 64, 255, 256, 257)
TIE_GAPS = (63, 64, 255, 256, 257)
# run lengths of test_device_trigger_scan_edge_cases: around one 64-sample block, one trip, two trips, a whole chunk
WALK_LENGTHS = (62, 63, 64, 65, 127, 128, 129, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP - 1, 2 * TRIP, 2 * TRIP + 1, CH - 1, CH, CH + 1)
RANDOM_SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025)


class Case(NamedTuple):
    name: str
    x: np.ndarray          # float32, read-only
    pairs: tuple           # the (thr_on, thr_off) pairs this trace is scanned at


def base(n=N, level=BASE):
    return np.full(n, level, np.float32)


def fill_run(x, start, length, filling, run=RUN, mid=MID):
    """A run of `length` samples from `start`: flat `run`, or `mid` with only the first / only the last sample at `run`."""
    x[start:start + length] = run if filling == "flat" else mid
    if filling == "first":
        x[start] = run
    elif filling == "last":
        x[start + length - 1] = run
    return x


def alternating(n=N, phase=0, level=BASE):
    x = base(n, level)
    x[phase::2] = RUN
    return x


def random_walk(rng, n, nan=False):
    """The family of test_device_trigger_scan_exact_on_random_traces."""
    x = np.clip(np.cumsum(rng.standard_normal(n)) * 0.15 + 0.3, 0, 1).astype(np.float32)
    if nan:
        x[rng.integers(0, n, size=max(1, n // 20))] = np.nan
    return x


def _families():
    yield "alt_even", alternating(phase=0), PAIRS
    yield "alt_odd", alternating(phase=1), PAIRS
    yield "alt_even_mid", alternating(phase=0, level=MID), PAIRS

    # run length x end position, the run at sample 0, the run open at the last sample
    for L in LENGTHS:
        places = [(f"e{e}", e - L + 1) for e in ENDS if e - L + 1 >= 0] + [("first", 0), ("last", N - L)]
        for where, start in places:
            for f in FILLINGS:
                yield f"run_L{L}_{where}_{f}", fill_run(base(), start, L, f), PAIRS

    # equal maxima: the peak is the FIRST one.  0.8 twice in a run at 0.7, `gap` apart: 64 and 256 meet in one lane of the
    # strided argmax (next load, next stride), 63 / 255 / 257 in two lanes (the wave reduction breaks the tie)
    start, L = CH - 100, 600  # crosses a chunk seam
    for d in TIE_OFFSETS:
        for gap in TIE_GAPS:
            x = fill_run(base(), start, L, "flat", run=LOW)
            x[start + d] = x[start + d + gap] = 0.8
            yield f"tie_d{d}_gap{gap}", x, PAIRS
    x = fill_run(base(), start, L, "flat", run=LOW)
    x[[start + d for d in TIE_OFFSETS]] = 0.8
    yield "tie_all_offsets", x, PAIRS
    x = fill_run(base(), start, L, "flat", run=LOW)
    x[start + L - 1] = 0.8
    yield "tie_last_only", x, PAIRS
    yield "tie_plateau", fill_run(base(), start, L, "flat", run=LOW), PAIRS  # every sample is a maximum

    # two-sample runs across the seams of phase 1's stride-256 loads, and across the chunk seam
    for seam in (256, 512, 768, 1024):
        x = base()
        x[CH + seam - 1:CH + seam + 1] = RUN
        yield f"stride_seam_{seam}", x, PAIRS
    x = base()
    for c in (0, 2 * CH):
        for seam in (256, 512, 768, 1024):
            if c + seam + 1 <= N:
                x[c + seam - 1:c + seam + 1] = RUN
    yield "stride_seams_all", x, PAIRS

    # values: the comparisons are strict, non-finite samples behave as in numpy
    x = fill_run(base(), 100, 50, "flat", run=MID)
    x[120] = 0.5  # == thr_on: no trigger under either pair
    x[300:310] = 0.5  # a run that only equals thr_on
    yield "equal_thr_on", x, PAIRS
    x = fill_run(base(), CH - 20, 50, "flat")
    x[CH] = 0.25  # == thr_off of the second pair: splits the run there (and below thr_off of the first)
    x[2000:2010] = 0.25
    yield "equal_thr_off", x, PAIRS
    x = fill_run(base(), CH - 20, 300, "flat")
    x[CH + 7] = np.inf
    x[CH + 200] = np.inf  # two equal maxima again
    yield "plus_inf_in_run", x, PAIRS
    x = fill_run(base(), CH - 70, 140, "flat")
    x[CH] = -np.inf
    yield "minus_inf_splits", x, PAIRS
    x = fill_run(base(), CH - 70, 140, "first")
    x[CH - 1] = np.nan
    x[CH + 30] = RUN
    yield "nan_splits", x, PAIRS
    x = fill_run(base(), 0, 30, "flat")
    x[0] = np.nan
    yield "nan_first_sample", x, PAIRS
    x = fill_run(base(), N - 30, 30, "flat")
    x[N - 1] = np.nan
    yield "nan_last_sample", x, PAIRS
    x = base(level=np.nan)
    yield "all_nan", x, PAIRS
    x = base(level=-1.5)
    fill_run(x, CH - 300, 600, "first", run=-0.6, mid=-1.1)
    fill_run(x, 2 * CH + 250, 10, "flat", run=-0.6)
    x[2 * CH + 300:2 * CH + 310] = -1.0  # == thr_on
    yield "negative_thresholds", x, ((-1.0, -1.0), (-1.0, -1.25))

    # the random-walk family of the random test, at the sizes around one trip and one chunk
    rng = np.random.default_rng(2024)
    for n in RANDOM_SIZES:
        for k in range(3):
            x = random_walk(rng, n, nan=(k == 2))
            thr = float(np.float32(rng.uniform(0.1, 0.8)))
            yield f"walk_n{n}_{k}", x, ((thr, thr), (thr, float(np.float32(thr / 2))))


@lru_cache(maxsize=None)
def all_cases():
    out = []
    for name, x, pairs in _families():
        x = np.ascontiguousarray(x, np.float32)
        x.setflags(write=False)
        out.append(Case(name, x, tuple(pairs)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in all_cases() if c.name == name)


@lru_cache(maxsize=None)
def expected():
    """{(case name, (thr_on, thr_off)): [(on, off, peak, value)]} by oracle.pipeline.picks_from_trace, computed once."""
    from oracle import pipeline as OP

    return {(c.name, p): OP.picks_from_trace(c.x, *p) for c in all_cases() for p in c.pairs}


def run_ends(x, thr_off, lo, hi):
    """Number of run ENDS inside [lo, hi): samples > thr_off whose next sample is not (or does not exist)."""
    above = np.asarray(x) > np.float32(thr_off)
    nxt = np.append(above[1:], False)
    return int(np.count_nonzero((above & ~nxt)[lo:hi]))


def same(got, want):
    """Two trigger lists [(on, off, peak, value)] are the same: indices as integers, values bit for bit."""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert tuple(int(v) for v in g[:3]) == tuple(int(v) for v in w[:3]), (g, w)
        assert np.float32(g[3]) == np.float32(w[3]), (g, w)
