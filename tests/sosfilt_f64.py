"""Inputs, the float64 answer, the bound and a host emulation of the scheme that the CPU and GPU tests of the device filter
share (volpick_amd/csrc/sosfilt.hip, ``vp_sos_filter``).  Numpy and scipy only; nothing here touches the device code.

Inputs: ``counts(n, seed)`` of tests/decimate_f64.py -- noise on a slow swing on an offset of 123456, which a high-pass has to
remove exactly.  Answer: ``filter_array(x.astype(float64), ...)`` from the product's own host module (scipy's sosfilt in
float64, what ObsPy computes).

Bound, on every sample: ``|got - want| <= 2^-22 max|x|``.  With float64 coefficients, state and intermediate the only error left
is the final rounding to float32, at most 2^-24 |y|; for the filters below on these inputs max|y| <= 1.19 max|x| (band-stop and
low-pass pass the offset, overshoot included), so the bound leaves a factor 3.3 over that rounding.  On the CPU
(tests/test_sosfilt_f64_cpu.py prints them) rounding ``want`` itself to float32 costs at most 0.26 of the bound and the float64
emulation of the carry scheme at most 1e-3 of it more.  No constant here was taken from a run of the kernel."""
import functools

import numpy as np

from tests.decimate_f64 import KINDS, TILE, bound, counts, ratio  # noqa: F401  (re-exported to the tests)
from volpick_amd.signal import butter_sos, filter_array

DF = 100.0
PIECE = 32  # samples per thread of the kernel (DC in sos_tile.h)
CARRY_WIDTH = 256  # tiles the carry launch scans at a time (DT in sosfilt.hip): the long trace must have more
FILTERS = {
    "highpass 0.3 Hz": ("highpass", dict(freq=0.3)),  # 2 sections, pole radius 0.9928
    "highpass 0.01 Hz": ("highpass", dict(freq=0.01)),  # pole radius 0.99976
    "highpass 1 Hz, 2 corners": ("highpass", dict(freq=1.0, corners=2)),  # 1 section
    "highpass 1 Hz, 3 corners": ("highpass", dict(freq=1.0, corners=3)),  # a first-order section
    "bandpass 1-20 Hz": ("bandpass", dict(freqmin=1.0, freqmax=20.0)),  # 4 sections
    "bandpass 0.05-45 Hz": ("bandpass", dict(freqmin=0.05, freqmax=45.0)),
    "lowpass 20 Hz": ("lowpass", dict(freq=20.0)),
    "bandstop 0.8-1.2 Hz": ("bandstop", dict(freqmin=0.8, freqmax=1.2)),
}
LENGTHS = (1, 31, 32, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 40_003)  # the kernel's seams: piece, tile
N_LONG = 300 * TILE + 77  # 301 tiles > CARRY_WIDTH: the carry launch's second chunk
assert N_LONG > CARRY_WIDTH * TILE


def sos_of(name):
    kind, opts = FILTERS[name]
    return butter_sos(kind, DF, **opts)


@functools.lru_cache(maxsize=None)
def trace(n):
    x = counts(n, 1000 + n % 997)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(name, n, zerophase):
    kind, opts = FILTERS[name]
    y = filter_array(trace(n), kind, DF, zerophase=zerophase, **opts)
    y.setflags(write=False)
    return y


def power_matrix(sos, span):
    """A^span (d x d, d = 2 sections), A the state after one zero sample from each unit state: the recurrence itself run over
    ``span`` zero samples.  State order s1, s2 per section, the order of scipy's ``zi``.  (The library squares A in double-double
    instead, volpick_amd/csrc/sos_matrices.h; squaring it in plain float64 is 5.7e-7 off at A^8192 for the 0.01 Hz high-pass,
    which alone costs a quarter of the bound.)"""
    from scipy.signal import sosfilt

    ns = len(sos)
    a = np.zeros((2 * ns, 2 * ns))
    for j in range(2 * ns):
        zi = np.zeros(2 * ns)
        zi[j] = 1.0
        _, zf = sosfilt(sos, np.zeros(span), zi=zi.reshape(ns, 2))
        a[:, j] = zf.reshape(-1)
    return a


def emulate(x, sos, zerophase=False, dtype=np.float64, carry="exact"):
    """The kernel's scheme on the host, arithmetic in ``dtype``, the result rounded to float32 at the end: pieces of 32 run from
    zero state; their ends carried through a tile with A^32 (from zero: the tile's end; from the tile's start state: every piece's
    start state); the tiles' ends carried with A^8192; every piece run again from its start state.  ``carry``: "exact"; "no_tile"
    (every tile starts from zero state); "no_piece" (every piece does)."""
    from scipy.signal import sosfilt

    sos = np.asarray(sos, dtype=np.float64)
    ns, d = len(sos), 2 * len(sos)
    m32, mtile = power_matrix(sos, PIECE).astype(dtype), power_matrix(sos, TILE).astype(dtype)
    sos_t = sos.astype(dtype)
    per_tile = TILE // PIECE

    def one_pass(u):
        n = len(u)
        npieces = -(-n // PIECE)
        pad = np.zeros(npieces * PIECE, dtype=dtype)
        pad[:n] = u
        pieces = pad.reshape(npieces, PIECE)
        _, zf = sosfilt(sos_t, pieces, axis=-1, zi=np.zeros((ns, npieces, 2), dtype=dtype))
        ends = zf.transpose(1, 0, 2).reshape(npieces, d)
        assert ends.dtype == dtype
        starts = np.zeros((npieces, d), dtype=dtype)
        z_tile = np.zeros(d, dtype=dtype)
        for t0 in range(0, npieces, per_tile):
            t1 = min(t0 + per_tile, npieces)
            e = np.zeros(d, dtype=dtype)  # the tile from zero state
            for p in range(t0, t1):
                e = m32 @ e + ends[p]
            z = z_tile.copy()
            for p in range(t0, t1):
                if carry != "no_piece":
                    starts[p] = z
                z = m32 @ z + ends[p]
            z_tile = mtile @ z_tile + e if carry == "exact" else np.zeros(d, dtype=dtype)
        y, _ = sosfilt(sos_t, pieces, axis=-1, zi=np.ascontiguousarray(starts.reshape(npieces, ns, 2).transpose(1, 0, 2)))
        assert y.dtype == dtype
        return y.reshape(-1)[:n]

    y = one_pass(np.asarray(x, dtype=dtype))
    if zerophase:
        y = one_pass(y[::-1])[::-1]
    return y.astype(np.float32)


def emulate_warmup(x, sos, zerophase=False, halo=1024, chunk=4096):
    """The scheme of the decimation kernel instead: every chunk run from zero state ``halo`` samples ahead of itself."""
    from scipy.signal import sosfilt

    def one_pass(u):
        out = np.empty(len(u))
        for c0 in range(0, len(u), chunk):
            c1 = min(c0 + chunk, len(u))
            s = max(0, c0 - halo)
            out[c0:c1] = sosfilt(sos, u[s:c1])[c0 - s:]
        return out

    y = one_pass(np.asarray(x, dtype=np.float64))
    if zerophase:
        y = one_pass(y[::-1])[::-1]
    return y.astype(np.float32)
