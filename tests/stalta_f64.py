"""Inputs, the float64 restatements, the extended-precision truth, the bars and a host emulation of the kernel's scheme that
the CPU and GPU tests of the device STA/LTA share (volpick_amd/csrc/stalta.hip, ``vp_sta_lta``).  Numpy only; nothing here
touches the device code.

Rule (include/volpick_hip.h has it in full), sq = x * x, tiny = the smallest normal double:
  recursive  sta = 0, lta = tiny, cft[0] = 0; for i >= 1: sta = csta sq[i] + (1 - csta) sta, lta likewise, cft[i] = sta / lta,
             replaced by 0 where i < nlta.
  classic    STA, LTA: window sums of sq over the last nsta, nlta samples divided by nsta, nlta; STA = 0 for i < nlta - 1;
             LTA below tiny is tiny; cft = STA / LTA.

Truth: the same rules in ``np.longdouble`` (80-bit on the build machines, eps 1.08e-19; asserted below), the classic windows
summed directly, sample by sample, never as a difference.

Bars, none taken from a run of the kernel.  Every term of these sums is non-negative, so a term that passes through D roundings
is off by at most D u relative, u = 2^-53:
  recursive, float64 out   |got - truth| <= (6 (i + 1) + 10) u truth at sample i: the sequential recursion's own worst case at 3
                           roundings per step and state.
  classic, float64 out     |got - truth| <= (nsta + nlta + 8) u truth: a window of w samples takes w - 1 additions.
  float32 out              the same plus 2^-24 truth.
  exact                    the zeroed head, an all-zero series (bit-equal 0), NaN placement.

The whole-trace cumulative-sum restatement of the classic type (what ObsPy computes) is held to the classic bar only on plain
counts; on the loud-then-quiet trace its running sum has swallowed the quiet samples and it misses the bar by orders of
magnitude -- tests/test_stalta_f64_cpu.py asserts that it does, so that the input keeps its point.
"""
import functools

import numpy as np

from tests.decimate_f64 import KINDS, TILE, counts  # noqa: F401  (re-exported to the tests)

U = 2.0 ** -53
TINY = float(np.finfo(np.float64).tiny)
PIECE = 32          # samples per thread of the kernel (DC in sos_tile.h)
CARRY_WIDTH = 256   # tiles the carry launch scans at a time (DT)
MAX_NLTA = 65536    # STALTA_MAX_NLTA
T, P = TILE, PIECE
assert np.finfo(np.longdouble).eps < 2e-19, "the truth needs an extended long double"

WINDOWS = ((1, 1), (5, 20), (50, 1000), (500, 2000), (1, T + 3), (T - 1, 2 * T + 1))
N_LONG = (CARRY_WIDTH + 3) * T + 77  # more tiles than the carry launch scans at a time


def seam_lengths(nlta):
    return sorted({n for n in (1, nlta - 1, nlta, nlta + 1, P - 1, P, P + 1, T - 1, T, T + 1, 2 * T + 5) if n >= 1})


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def plain(n):
    x = counts(n, 2000 + n % 991)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def loud_then_quiet(n):
    """``counts`` minus its offset, 400 samples in the middle 10^4 times louder: behind them a whole-trace running sum of squares
    is 10^8 times a quiet window's sum."""
    x = counts(n, 2000 + n % 991) - 123456.0
    x[n // 2:n // 2 + 400] *= 1e4
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def zeros_then_noise(n, lead):
    """``lead`` zeros, then noise: with lead >= nlta the classic cft at sample ``lead`` is exactly nlta / nsta."""
    x = np.zeros(n)
    x[lead:] = np.round(800.0 * np.random.default_rng(7).standard_normal(n - lead))
    x[lead] = 801.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def bursts(n):
    """The trigger cases' input: integer noise with a burst eight times louder every 3000 samples, the last one open at the end."""
    x = np.round(800.0 * np.random.default_rng(11 + n).standard_normal(n))
    for at in list(range(1500, n - 300, 3000)) + [max(n - 40, 0)]:
        x[at:at + 300] *= 8.0
    x.setflags(write=False)
    return x


# (kind, n, nsta, nlta, thr_on, thr_off) on ``bursts(n)``: the reference's thresholds; tests/test_stalta_f64_cpu.py asserts of
# every one that no truth sample lies within its bar of a threshold
TRIGGER_CASES = (("recursive", 2 * T + 5, 5, 20, 2.0, 0.5), ("classic", 2 * T + 5, 5, 20, 2.0, 0.5),
                 ("recursive", 40_003, 500, 2000, 2.0, 0.5), ("classic", 40_003, 50, 1000, 2.0, 0.5))

INPUTS = {"plain": plain, "loud_then_quiet": loud_then_quiet}
ALL_INPUTS = dict(INPUTS, bursts=bursts)


# -------------------------------------------------------------------------------------------- float64 restatements
def recursive64(x, nsta, nlta):
    """``recursive_sta_lta_py`` as the loop it is."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    csta, clta = 1.0 / nsta, 1.0 / nlta
    sta, lta = 0.0, TINY
    cft = np.zeros(n)
    sq = (x * x).tolist()
    for i in range(1, n):
        sta = csta * sq[i] + (1.0 - csta) * sta
        lta = clta * sq[i] + (1.0 - clta) * lta
        cft[i] = 0.0 if sta == 0.0 else sta / lta  # (0 / lta also where tiny (1 - clta)^i has left the doubles)
    cft[:min(nlta, n)] = 0.0
    return cft


def classic64(x, nsta, nlta):
    """``classic_sta_lta_py`` as the cumulative sum it is."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    sta = np.cumsum(x * x)
    lta = sta.copy()
    sta[nsta:] = sta[nsta:] - sta[:-nsta]
    sta /= nsta
    lta[nlta:] = lta[nlta:] - lta[:-nlta]
    lta /= nlta
    sta[:min(nlta - 1, n)] = 0.0
    lta[lta < TINY] = TINY
    return sta / lta


def cumsum_bound(x, nsta, nlta):
    """The cumulative-sum restatement's own rounding bound, propagated to the ratio: each running sum S_i is off by at most
    2 (i + 1) u S_i (one square, one addition per term), a window by twice that; relative to the window sums themselves."""
    x = np.asarray(x, dtype=np.longdouble)
    s = np.cumsum(x * x)
    i = np.arange(len(x), dtype=np.longdouble)
    err = 4 * (i + 1) * U * s
    ws, wl = window_sums(x * x, nsta), window_sums(x * x, nlta)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = err / ws + err / wl
    return np.where(np.isfinite(rel), rel, 0).astype(np.float64)


# -------------------------------------------------------------------------------------------------------------- truth
def window_sums(sq, w):
    """sum of sq over the w samples ending at i (fewer at the start), each window summed directly in sq's dtype."""
    n = len(sq)
    pad = np.concatenate([np.zeros(w - 1, dtype=sq.dtype), sq])
    out = np.empty(n, dtype=sq.dtype)
    view = np.lib.stride_tricks.sliding_window_view(pad, w)
    step = max(1, (1 << 22) // w)
    for i0 in range(0, n, step):
        out[i0:i0 + step] = view[i0:i0 + step].sum(axis=1)
    return out


@functools.lru_cache(maxsize=64)
def _truth(kind, name, n, nsta, nlta, lead=0):
    x = (zeros_then_noise(n, lead) if name == "zeros_then_noise" else ALL_INPUTS[name](n)).astype(np.longdouble)
    y = classic_truth(x, nsta, nlta) if kind == "classic" else recursive_truth(x, nsta, nlta)
    y.setflags(write=False)
    return y


def truth(kind, name, n, nsta, nlta, lead=0):
    return _truth(kind, name, n, nsta, nlta, lead)


def recursive_truth(x, nsta, nlta):
    L = np.longdouble
    x = np.asarray(x, dtype=L)
    n = len(x)
    one = L(1)
    csta, clta = one / L(nsta), one / L(nlta)
    asta, alta = one - csta, one - clta
    sta, lta = L(0), L(TINY)
    cft = np.zeros(n, dtype=L)
    sq = x * x
    for i in range(1, n):
        s = sq[i]
        sta = csta * s + asta * sta
        lta = clta * s + alta * lta
        if sta != 0:
            cft[i] = sta / lta
    cft[:min(nlta, n)] = 0
    return cft


def classic_truth(x, nsta, nlta):
    L = np.longdouble
    x = np.asarray(x, dtype=L)
    n = len(x)
    sq = x * x
    sta = window_sums(sq, nsta) / L(nsta)
    lta = window_sums(sq, nlta) / L(nlta)
    sta[:min(nlta - 1, n)] = 0
    lta[lta < L(TINY)] = L(TINY)
    return sta / lta


# --------------------------------------------------------------------------------------------------------------- bars
def bar(kind, t, nsta, nlta, out32=False):
    t = np.abs(np.asarray(t, dtype=np.longdouble))
    if kind == "classic":
        d = np.longdouble(nsta + nlta + 8)
    else:
        d = 6 * (np.arange(len(t), dtype=np.longdouble) + 1) + 10
    return (d * U + (2.0 ** -24 if out32 else 0.0)) * t


def ratio(kind, got, t, nsta, nlta, out32=False):
    """Worst |got - truth| / bar over every sample; a sample whose bar is 0 must be exactly the truth (inf otherwise), and so
    must the shapes and the NaNs."""
    got = np.asarray(got)
    if got.shape != t.shape:
        return float("inf")
    g = got.astype(np.longdouble)
    if not np.array_equal(np.isnan(g), np.isnan(t)):
        return float("inf")
    ok = ~np.isnan(t)
    d = np.abs(g[ok] - t[ok])
    b = bar(kind, t, nsta, nlta, out32)[ok]
    if np.any(d[b == 0] != 0):
        return float("inf")
    nz = b > 0
    return float((d[nz] / b[nz]).max()) if nz.any() else 0.0


def clear_of_thresholds(kind, t, nsta, nlta, thr_on, thr_off):
    """No truth sample lies within its float32 bar, plus the rounding of a float32 host value, of either threshold; within
    every trigger the largest sample stands clear of the others by as much.  Asserted for every trigger case the tests use."""
    t = np.asarray(t, dtype=np.longdouble)
    b = 2 * bar(kind, t, nsta, nlta, out32=True)
    for thr in (thr_on, thr_off):
        close = np.abs(t - np.float32(thr)) <= b
        assert not close.any(), f"{int(close.sum())} samples within their bar of threshold {thr}"
    above = t > thr_off
    edges = np.flatnonzero(np.diff(np.concatenate([[False], above, [False]]).astype(np.int8)))
    for lo, hi in zip(edges[::2], edges[1::2]):
        hit = np.flatnonzero(t[lo:hi] > thr_on)
        if len(hit) == 0:
            continue
        run = t[lo + hit[0]:hi]
        k = int(np.argmax(run))
        others = np.delete(run, k)
        assert len(others) == 0 or run[k] - others.max() > 2 * b[lo + hit[0] + k], "two peaks within the bar of each other"


# ---------------------------------------------------------------------------------- the kernel's scheme on the host
def _pow(a, k):
    return float(np.longdouble(a) ** k)


def emulate_recursive(x, nsta, nlta, carry="exact"):
    with np.errstate(invalid="ignore"):  # (0 * NaN: a non-finite sample stays in the state through every product)
        return _emulate_recursive(x, nsta, nlta, carry)


def _emulate_recursive(x, nsta, nlta, carry):
    """Pieces of 32 steps run from zero state; their ends carried through a tile with a^32 and the tiles' ends with a^8192,
    lta's start value tiny as the first tile's state; every piece run again from its start state.  float64.  ``carry``:
    "exact"; "no_tile" (every tile but the first starts from zero state); "no_piece" (every piece does)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    cft = np.zeros(n)
    if n < 2:
        return cft
    c = np.array([1.0 / nsta, 1.0 / nlta])
    a = 1.0 - c
    a32 = np.array([_pow(a[0], P), _pow(a[1], P)])
    aT = np.array([_pow(a[0], T), _pow(a[1], T)])
    steps = n - 1
    npieces = -(-steps // P)
    sq = np.zeros(npieces * P)
    sq[:steps] = x[1:] * x[1:]
    pieces = sq.reshape(npieces, P)

    def run(state):  # state (npieces, 2) -> every step's (sta, lta), the end state
        out = np.empty((npieces, P, 2))
        s = state.copy()
        for i in range(P):
            s = c * pieces[:, i:i + 1] + a * s
            out[:, i] = s
        return out, s

    _, ends = run(np.zeros((npieces, 2)))
    starts = np.zeros((npieces, 2))
    per_tile = T // P
    z_tile = np.array([0.0, TINY])
    for t0 in range(0, npieces, per_tile):
        t1 = min(t0 + per_tile, npieces)
        e = np.zeros(2)
        for p in range(t0, t1):
            e = a32 * e + ends[p]
        z = z_tile.copy()
        for p in range(t0, t1):
            starts[p] = z if (carry != "no_piece" or p == 0) else 0.0
            z = a32 * z + ends[p]
        z_tile = aT * z_tile + e if carry != "no_tile" else np.zeros(2)
    out, _ = run(starts)
    sta, lta = out[..., 0].reshape(-1)[:steps], out[..., 1].reshape(-1)[:steps]
    with np.errstate(invalid="ignore", divide="ignore"):
        np.divide(sta, lta, out=cft[1:], where=sta != 0.0)
    cft[:min(nlta, n)] = 0.0
    return cft


def _segmented(sq, w, rev, carry):
    """P (forward) or S (``rev``) of the classic scheme: running sums that start anew on every block edge of width w, built
    piece by piece and tile by tile as the kernel builds them."""
    n = len(sq)
    nt = -(-n // T)
    pad = np.zeros(nt * T)
    pad[:n] = sq
    pos = np.arange(nt * T)
    if rev:
        pos = pos.reshape(nt, T)[::-1, ::-1].reshape(-1)  # the order of work: last tile first, each right to left
    v = pad[pos].reshape(-1, P)
    edge = ((pos % w) == (w - 1 if rev else 0)).reshape(-1, P)
    loc = np.empty_like(v)
    seen = np.zeros_like(edge)
    acc = np.zeros(len(v))
    got = np.zeros(len(v), dtype=bool)
    for i in range(P):
        acc = np.where(edge[:, i], 0.0, acc) + v[:, i]
        got = got | edge[:, i]
        loc[:, i] = acc
        seen[:, i] = got
    running = 0.0
    per_tile = T // P
    for p in range(len(v)):
        if p % per_tile == 0 and carry == "no_tile":
            running = 0.0
        ahead = 0.0 if carry == "no_piece" else running
        running = acc[p] if got[p] else running + acc[p]
        loc[p] = np.where(seen[p], loc[p], ahead + loc[p])
    out = np.empty(nt * T)
    out[pos] = loc.reshape(-1)
    return out[:n]


def emulate_classic(x, nsta, nlta, carry="exact"):
    """Every window as S[i - w + 1] + P[i], never a difference.  float64.  ``carry`` as in :func:`emulate_recursive`."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    bad = ~np.isfinite(x)
    sq = np.where(bad, np.nan, x) ** 2
    i = np.arange(n)

    def window(w):
        p, s = _segmented(sq, w, False, carry), _segmented(sq, w, True, carry)
        use = (i >= w) & ((i + 1) % w != 0)
        return np.where(use, s[np.maximum(i - w + 1, 0)] + p, p)

    sta, lta = window(nsta) / nsta, window(nlta) / nlta
    sta[:min(nlta - 1, n)] = 0.0
    lta[lta < TINY] = TINY
    cft = sta / lta
    if bad.any():
        cft[int(np.argmax(bad)):] = np.nan
    return cft
