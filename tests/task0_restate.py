"""The threshold sweep of task 0 (csrc/sweep.hip, vp_sweep_*) restated in numpy, and the probabilities it is tried on.

The rule is ObsPy's ``trigger_onset`` as ``oracle.pipeline`` states it, on the border slice, with float32 thresholds (a
float32 array compared with a ``np.float32`` scalar compares in float32 under NumPy 1 and 2 alike), then per trigger the
FIRST argmax of ``[on, off]`` and the value AT it.  Not a test module."""
import functools

import numpy as np

from oracle.pipeline import trigger_onset

GRID = np.arange(0.1, 1.0, 0.1)  # the reference's prob_thres


def thresholds(grid):
    """-> (thr_on, thr_off) float32, thr_off = thr_on / 2."""
    on = np.ascontiguousarray(np.asarray(grid, np.float64).astype(np.float32))
    return on, np.ascontiguousarray(on / np.float32(2))


def picks(x, on, off):
    """x: a float32 border slice -> (peaks, values) of every trigger, ascending."""
    x = np.asarray(x, np.float32)
    on, off = np.float32(on), np.float32(off)
    peaks = [int(s0 + np.argmax(x[s0:s1 + 1])) for s0, s1 in trigger_onset(x, on, off)]
    return np.array(peaks, np.int64), x[np.array(peaks, np.int64)]


def sweep(prob, p_row, s_row, thr_on, thr_off, K, lo=None, hi=None):
    """-> count (B, 2, NT) int32, peak (B, 2, NT, K) int32 (-1 behind the count), value float32 (0 behind the count)."""
    B, _, T = prob.shape
    NT = len(thr_on)
    count = np.zeros((B, 2, NT), np.int32)
    peak = np.full((B, 2, NT, K), -1, np.int32)
    value = np.zeros((B, 2, NT, K), np.float32)
    for b in range(B):
        a, e = (0, T) if lo is None else (int(lo[b]), int(hi[b]))
        for ph, row in enumerate((p_row, s_row)):
            x = prob[b, row, a:e]
            for j in range(NT):
                pk, v = picks(x, thr_on[j], thr_off[j])
                count[b, ph, j] = len(pk)
                peak[b, ph, j, :len(pk[:K])] = pk[:K]
                value[b, ph, j, :len(pk[:K])] = v[:K]
    return count, peak, value


def same(got, want):
    """Bit for bit: (count, peak, value or None) against sweep()'s triple."""
    ok = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if got[2] is not None:
        ok = ok and np.array_equal(np.asarray(got[2]).view(np.uint32), want[2].view(np.uint32))
    return ok


# ---- adversarial rows ----------------------------------------------------------------------------------------------------
# Every kind writes one row of T samples around one threshold pair (on, off) and the border [a, e); rows are float32 and
# stay inside [0, 1] but for the NaN.
def _between(rng, n, off, on):
    """n values strictly between off and on."""
    v = (off + (on - off) * (0.1 + 0.8 * rng.random(n))).astype(np.float32)
    assert ((v > off) & (v < on)).all()
    return v


def _above(rng, n, on):
    v = (on + (1 - on) * (0.05 + 0.9 * rng.random(n))).astype(np.float32)
    assert (v > on).all()
    return v


def _quiet(rng, x, a, e, on, off):
    x[:] = (off * 0.99 * rng.random(len(x))).astype(np.float32)
    x[a] = off  # exactly the off threshold: not above it


def _between_only(rng, x, a, e, on, off):
    for s in range(a, e, 97):
        n = min(40, e - s)
        x[s:s + n] = _between(rng, n, off, on)


def _plateau_at_on(rng, x, a, e, on, off):
    m = (a + e) // 2
    s, t = max(a, m - 60), min(e, m + 60)
    x[s:t] = _between(rng, t - s, off, on)
    x[max(s, m - 10):min(t, m + 10)] = on  # the strict > rejects it


def _whole(rng, x, a, e, on, off):
    x[:] = _between(rng, len(x), off, on)
    x[a + (e - a) // 3] = _above(rng, 1, on)[0]
    x[a + 2 * (e - a) // 3:] = np.maximum(x[a + 2 * (e - a) // 3:], np.float32(0.5) * (on + 1))


def _cut_lo(rng, x, a, e, on, off):
    s, t = max(0, a - 50), min(e, a + 30)
    x[s:t] = _above(rng, t - s, on)
    if a > 0:
        x[a - 1] = 1.0  # the run's maximum lies in front of the border


def _cut_hi(rng, x, a, e, on, off):
    s, t = max(a, e - 30), min(len(x), e + 50)
    x[s:t] = _above(rng, t - s, on)
    if e < len(x):
        x[e] = 1.0  # ... and behind it


def _edge_peaks(rng, x, a, e, on, off):
    x[a] = x[e - 1] = 1.0
    if e - a > 4:
        x[a + 1] = x[e - 2] = _between(rng, 1, off, on)[0]


def _two_bumps(rng, x, a, e, on, off):
    m = (a + e) // 2
    s, t = max(a, m - 100), min(e, m + 100)
    x[s:t] = _between(rng, t - s, off, on)  # one off-run; its first bump stays below on
    if t - s > 20:
        x[t - 15:t - 10] = _above(rng, 5, on)


def _equal_maxima(rng, x, a, e, on, off):
    s, t = a, min(e, a + 900)
    x[s:t] = _between(rng, t - s, off, on)
    top = _above(rng, 1, on)[0]
    x[min(t - 1, s + 150)] = top
    x[min(t - 1, s + 550)] = top  # 400 samples on: another wave's, the lowest index wins


def _nan_in_run(rng, x, a, e, on, off):
    m = (a + e) // 2
    s, t = max(a, m - 80), min(e, m + 80)
    x[s:t] = _above(rng, t - s, on)
    x[m] = np.nan  # ends the run: two triggers


def _single_gap(rng, x, a, e, on, off):
    s = a
    while s < min(e, a + 400):
        n = min(int(rng.integers(1, 20)), e - s)
        x[s:s + n] = _above(rng, n, on)
        s += n + 1  # one sample at or below off between the runs
        if s - 1 < e:
            x[s - 1] = off if rng.random() < 0.5 else 0.0


def _spikes(rng, x, a, e, on, off):
    s = a
    while s < e:  # run ends on every residue of every chunk length; far more triggers than K
        x[s] = _above(rng, 1, on)[0]
        s += int(rng.integers(1, 31))


def _random(rng, x, a, e, on, off):
    v = rng.random(len(x) + 8) ** 3
    x[:] = np.convolve(v, np.ones(9) / 9, "valid").astype(np.float32) * 2.5
    np.clip(x, 0, 1, out=x)


ROW_KINDS = (_quiet, _between_only, _plateau_at_on, _whole, _cut_lo, _cut_hi, _edge_peaks, _two_bumps, _equal_maxima,
             _nan_in_run, _single_gap, _spikes, _random)


def border_cases(T):
    return [(0, T), (1, T), (0, T - 1), (3, 1003), (T - 1000, T), (T // 2 - 1, T // 2 + 2), (7, 8), (T - 1, T), (2, 3000),
            (T - 3000, T - 1), (255, 2 * 256 + 1), (13 * 19, T - 25 * 3),
            (5, 5 + 13 * 25 * 2), (300, 300 + 13 * 25 * 8)]  # whole chunks of 13 and of 25 samples: no thread is cut short


def adversarial_batch(T, B, seed, p_row, s_row, n_rows=3, grid=GRID):
    """(prob (B, n_rows, T) float32, lo, hi): window b has border case b, its P row kind b and its S row kind b + 5, each
    written around one threshold pair of ``grid`` (in turn); the other rows are noise."""
    rng = np.random.default_rng(seed)
    on, off = thresholds(grid)
    prob = (0.04 * rng.random((B, n_rows, T))).astype(np.float32)
    cases = border_cases(T)
    lo, hi = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        a, e = cases[(b + seed) % len(cases)]
        lo[b], hi[b] = a, e
        for k, row in ((b, p_row), (b + 5, s_row)):
            j = (b + k + seed) % len(on)
            x = np.zeros(T, np.float32)
            ROW_KINDS[k % len(ROW_KINDS)](rng, x, a, e, on[j], off[j])
            prob[b, row] = x
    return prob, lo, hi


@functools.lru_cache(maxsize=None)
def adversarial_case(T, B, seed, p_row, s_row, borders=True):
    """The batch and its sweep at the widest shape the tests ask for -- NT = 32, K = 64 -- computed once per session;
    ``narrowed`` cuts every smaller case out of it.  Nothing here is written to afterwards."""
    prob, lo, hi = adversarial_batch(T, B, seed, p_row, s_row)
    on, off = thresholds(WIDE_GRID)
    want = sweep(prob, p_row, s_row, on, off, 64, *((lo, hi) if borders else (None, None)))
    for arr in (prob, lo, hi) + want:
        arr.setflags(write=False)
    return prob, lo, hi, want


# 32 thresholds that hold the reference's nine (as float32) among them: the nine first, then 23 more.
WIDE_GRID = np.concatenate([GRID, np.linspace(0.02, 0.98, 23)])


def narrowed(want, NT, K):
    """The sweep of the first NT thresholds with K slots, from the one with 32 thresholds and 64 slots."""
    count, peak, value = want
    return count[:, :, :NT].copy(), peak[:, :, :NT, :K].copy(), value[:, :, :NT, :K].copy()
