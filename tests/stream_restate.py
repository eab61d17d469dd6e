"""The stream assembly rule of ``volpick_amd.models._group_stream`` / ``_zero_filled``, restated from its description with
numpy and the standard library only (no torch, nothing of the package), and a seeded generator of irregular layouts.

A layout is a list of traces ``(network, station, location, channel, start_us, samples)``: ``start_us`` integer microseconds
since the epoch, ``samples`` a 1-D numpy array (int32 / float32 / float64, possibly masked).  The rule:

* an instrument is ``(network, station, location, channel[:-1])``; instruments come out sorted by that key;
* the component is the last channel letter; a letter outside ``component_order`` is looked up in 1 -> N, 2 -> E, 3 -> Z; a
  piece whose component is still unknown covers samples (it extends runs) and writes none;
* a piece begins at sample ``round((start_us - earliest start_us of the instrument) * rate / 1e6)``;
* runs are the union of ``[s0, s0 + len)`` over the pieces with ``len > 0``, abutting pieces merged; a run shorter than
  ``in_samples`` is dropped; every other run is one block;
* inside a block every cell of a component holds the sample of the LONGEST trace of that component that covers it, among
  equally long ones of the one LATER in the stream; cells nobody covers and masked samples are 0; a value becomes float32
  once, straight from its own dtype;
* the block starts at ``earliest start_us + round(b0 / rate * 1e6)``.

Times are exact: integers and ``fractions.Fraction`` (whose ``round`` is half to even, as Python's is for floats); no float
ever holds a time.  The cell rule is a per-cell maximum of ``(length, position in the stream)``, which does not depend on
the order in which pieces are visited -- the code under test gets there by writing pieces in ascending length.
"""
from fractions import Fraction

import numpy as np

ALIAS = {"1": "N", "2": "E", "3": "Z"}
COMPONENT_SETS = ("ZNE", "Z12", "312", "Z", "ZN", "ZNEX")
DTYPES = (np.float32, np.float64, np.int32)


def _instruments(layout):
    groups = {}
    for pos, (net, sta, loc, cha, start_us, samples) in enumerate(layout):
        groups.setdefault((net, sta, loc, cha[:-1]), []).append((pos, cha[-1:] if cha else "", int(start_us), samples))
    return sorted(groups.items())


def _component(letter, component_order):
    if letter == "":  # (no channel code at all: not a case the layouts hold)
        return -1
    if letter not in component_order:
        letter = ALIAS.get(letter, letter)
    return component_order.index(letter) if letter in component_order else -1


def _blocks(layout, component_order, sampling_rate, in_samples):
    """``(blocks, dropped)``.  One dict per block: trace_id, start_us, data (C, N) float32, fast (every component is exactly
    one trace that spans the block, and no other trace of a known component touches it); ``dropped``: how many runs were
    shorter than ``in_samples``."""
    rate = Fraction(sampling_rate)
    n_comp = len(component_order)
    out, dropped = [], 0
    for (net, sta, loc, _), traces in _instruments(layout):
        t_start = min(start_us for _, _, start_us, _ in traces)
        pieces = []  # (first sample, length, component or -1, position in the stream, samples)
        for pos, letter, start_us, samples in traces:
            s0 = round(Fraction(start_us - t_start) * rate / 1_000_000)
            pieces.append((s0, len(samples), _component(letter, component_order), pos, samples))
        runs = []
        for s0, n, _, _, _ in sorted(pieces, key=lambda p: p[0]):
            if n <= 0:
                continue
            if runs and s0 <= runs[-1][1]:
                runs[-1][1] = max(runs[-1][1], s0 + n)
            else:
                runs.append([s0, s0 + n])
        for b0, b1 in runs:
            if b1 - b0 < in_samples:
                dropped += 1
                continue
            data = np.zeros((n_comp, b1 - b0), np.float32)
            best = np.full((n_comp, b1 - b0), -1, np.int64)  # rank of the trace whose sample the cell holds
            touching = []
            for s0, n, c, pos, samples in pieces:
                lo, hi = max(s0, b0), min(s0 + n, b1)
                if c < 0 or hi <= lo:
                    continue
                touching.append((c, s0 == b0 and n == b1 - b0))
                values = np.ma.filled(samples, 0) if np.ma.isMaskedArray(samples) else np.asarray(samples)
                values = values[lo - s0:hi - s0].astype(np.float32)
                rank = n * (len(layout) + 1) + pos  # longer first, then later in the stream
                wins = rank > best[c, lo - b0:hi - b0]
                data[c, lo - b0:hi - b0][wins] = values[wins]
                best[c, lo - b0:hi - b0][wins] = rank
            fast = sorted(touching) == [(c, True) for c in range(n_comp)]
            out.append(dict(trace_id=f"{net}.{sta}.{loc}", start_us=t_start + round(Fraction(b0 * 1_000_000) / rate), data=data,
                            fast=fast))
    return out, dropped


def restate(layout, component_order="ZNE", sampling_rate=100, in_samples=3001):
    """[(trace_id, block_start_us, float32 (C, N) array)], instruments sorted, runs ascending."""
    return [(b["trace_id"], b["start_us"], b["data"]) for b in _blocks(layout, component_order, sampling_rate, in_samples)[0]]


def full_rows(layout, component_order="ZNE", sampling_rate=100, in_samples=3001):
    """One bool per block of ``restate``: the block is nothing but one full-length trace per component."""
    return [b["fast"] for b in _blocks(layout, component_order, sampling_rate, in_samples)[0]]


def short_runs(layout, component_order="ZNE", sampling_rate=100, in_samples=3001):
    """How many runs ``restate`` dropped as shorter than ``in_samples``: one warning each in the code under test."""
    return _blocks(layout, component_order, sampling_rate, in_samples)[1]


# --------------------------------------------------------------------------- seeded irregular layouts
def _values(rng, n, dtype):
    if dtype is np.int32:  # counts; half of the traces beyond 2^24, where float32 no longer holds every integer
        top = 2**30 if rng.random() < 0.5 else 2**20
        return rng.integers(-top, top, n).astype(np.int32)
    x = rng.standard_normal(n) * 1e3
    return x.astype(np.float32) if dtype is np.float32 else x  # float64 values that float32 rounds


def random_layout(rng, scale, sampling_rate=100, origin_us=1_600_000_000_000_000):
    """1-4 stations; per station a component set of ``COMPONENT_SETS`` and either one full-length trace per component (one in
    five) or 1-3 pieces per component that overlap, abut or leave a gap, now and then with an equally long rival; lengths
    from 1 sample to ~2.3 ``scale``; starts off the sample grid by at most 0.2 sample (never by half a sample: there the
    rounding is a convention); dtype drawn per trace; traces shuffled."""
    us = Fraction(1_000_000) / Fraction(sampling_rate)
    traces = []
    jitter = lambda: int(rng.integers(-int(us / 5), int(us / 5) + 1))  # noqa: E731
    at = lambda s: origin_us + int(s * us) + jitter()  # noqa: E731
    length = lambda: int(rng.integers(1, scale // 8 + 2)) if rng.random() < 0.15 else int(rng.integers(scale // 3, int(2.3 * scale) + 1))  # noqa: E731
    names = rng.permutation(100)
    for k in range(int(rng.integers(1, 5))):
        comps = COMPONENT_SETS[int(rng.integers(len(COMPONENT_SETS)))]
        sta, loc = f"S{int(names[k]):02d}", ("", "00")[int(rng.integers(2))]
        first = int(rng.integers(0, 50))

        def add(letter, s0, n):
            traces.append(("XX", sta, loc, "HH" + letter, at(s0), _values(rng, n, DTYPES[int(rng.integers(3))])))

        if rng.random() < 0.2:
            n = int(rng.integers(scale, int(2.3 * scale) + 1))
            for letter in comps:
                add(letter, first, n)
            continue
        for letter in comps:
            end = first + int(rng.integers(0, scale // 4 + 1))
            for i in range(int(rng.integers(1, 4))):
                n = length()
                how = int(rng.integers(3)) if i else 1
                s0 = end - int(rng.integers(1, scale // 2 + 1)) if how == 0 else end if how == 1 else end + int(rng.integers(1, scale // 2 + 1))
                add(letter, s0, n)
                if rng.random() < 0.15:  # an equally long trace over (part of) the same samples: the later one wins
                    add(letter, s0 + int(rng.integers(0, n // 2 + 1)), n)
                end = s0 + n
    return [traces[i] for i in rng.permutation(len(traces))]
