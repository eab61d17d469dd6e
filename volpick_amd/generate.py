"""PhaseNet training batches generated on the GPU from a device-resident waveform bank.

The reference builds its training batches with SeisBench generators.  Every one of its training configs uses the core
list of ``PhaseNetLit.get_joint_augmentation_block1`` (the reference's volpick/model/models.py:221-265):

1. ``OneOf([WindowAroundSample(samples_before=3000, windowlen=6000, selection="random", strategy="pad"), Null], [2, 1])``
2. ``RandomWindow(windowlen=3001, strategy="pad")``
3. ``ProbabilisticLabeller(shape="gaussian", sigma)`` with volpick's ``phase_dict`` (models.py:26-31)
4. ``Normalize(demean_axis=-1, amp_norm_axis=-1, amp_norm_type=model.norm)``
5. ``ChangeDtype(float32)``

The work is split in two.  :class:`WindowPlanner` draws every random choice of steps 1-2 on the host and writes one plan
row ``(trace, start, lo, hi)`` per window: ``x[c][t] = bank[trace][c][start + t]`` where ``lo <= start + t < hi``, else 0.
The GPU executes the rows (``vp_bank_make_batch``, ``vp_train_step_bank``): one kernel cuts, demeans, normalises and
labels the whole batch from a :class:`WaveformBank` that stays in device memory.

SeisBench is not available to pin the generator semantics below; each choice that rests on its behaviour is one named
constant here:

* ``NO_PICK_FALLBACK`` -- what the around-a-pick branch does with a trace that has no finite onset;
* ``PAD_LEFT_AT_NEGATIVE_P0`` -- how a window that starts before the trace (``p0 < 0``) is filled;
* ``P0_ROUNDING`` -- how ``onset - samples_before`` becomes an integer sample;
* ``NOISE_RULE`` -- the noise label where the P and S Gaussians overlap.

Out of scope: volpick's stacking augmentations (``get_stack_block``), ``AddGap``, array rotation and the second
``Normalize`` they make necessary.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

# --- generator semantics SeisBench would pin -----------------------------------------------------------------------
NO_PICK_FALLBACK = "null"   # around-a-pick branch on a trace without a finite onset: "null" (take the null branch) or "error"
PAD_LEFT_AT_NEGATIVE_P0 = True  # p0 < 0: zeros in front of the trace (lo = 0); False: the extent starts at sample 0 instead
P0_ROUNDING = np.trunc      # p0 = int(onset - samples_before): truncation toward zero
NOISE_RULE = "clip"         # noise = clip(1 - P - S, 0, 1); overlapping P and S are not rescaled (fixed in the kernel)

# the reference's phase_dict (volpick/model/models.py:26-31): metadata column -> phase, two columns per phase
PHASE_DICT = {
    "trace_p_arrival_sample": "P",
    "trace_P_arrival_sample": "P",
    "trace_s_arrival_sample": "S",
    "trace_S_arrival_sample": "S",
}

PLAN_ROW = np.dtype([("trace", np.int32), ("reserved", np.int32), ("start", np.int64), ("lo", np.int64), ("hi", np.int64)],
                    align=True)
assert PLAN_ROW.itemsize == C.sizeof(_lib.VpPlanRow)


def as_rows(rows) -> np.ndarray:
    """A contiguous PLAN_ROW array (a PLAN_ROW array or anything with trace / start / lo / hi fields)."""
    rows = np.asarray(rows)
    if rows.dtype != PLAN_ROW:
        if rows.dtype.names is None or not {"trace", "start", "lo", "hi"} <= set(rows.dtype.names):
            raise TypeError("plan rows need the fields trace, start, lo, hi (generate.PLAN_ROW)")
        out = np.zeros(rows.shape, PLAN_ROW)
        for k in ("trace", "start", "lo", "hi"):
            out[k] = rows[k]
        rows = out
    if rows.ndim != 1 or rows.size == 0:
        raise ValueError("plan rows: a non-empty 1-D array")
    return np.ascontiguousarray(rows)


def label_rows(labels) -> np.ndarray:
    """Output row of P, S and noise for a model's ``labels`` (e.g. "PSN" or "NPS")."""
    labels = "".join(labels)
    if sorted(labels) != ["N", "P", "S"]:
        raise ValueError(f"labels must be a permutation of 'PSN', got {labels!r}")
    return np.array([labels.index("P"), labels.index("S"), labels.index("N")], np.int32)


def _onset_table(onsets, n):
    """{"P": (N,) or (N, 2), "S": ...} -> (N, 4) float64: P, P, S, S (NaN = no pick)."""
    out = np.full((n, 4), np.nan)
    for col, phase in ((0, "P"), (2, "S")):
        if phase not in onsets or onsets[phase] is None:
            continue
        a = np.asarray(onsets[phase], np.float64)
        if a.ndim == 1:
            a = a[:, None]
        if a.shape[0] != n or a.shape[1] > 2:
            raise ValueError(f"onsets[{phase!r}]: expected ({n},) or ({n}, 2), got {a.shape}")
        out[:, col:col + a.shape[1]] = a
    return out


class WaveformBank:
    """A set of three-component traces in device memory, each stored as (3, L_i) fp32 in the model's component order
    with up to two P and two S onsets (trace samples; NaN = no pick).

    ``waveforms``: a list of (3, L_i) arrays, an (N, 3, L) array, or an (N, 3, L) CUDA tensor (copied device to device).
    ``onsets``: ``{"P": (N,) or (N, 2), "S": ...}``."""

    CHUNK_FLOATS = 1 << 26  # host data is written in chunks of about this many floats (256 MB)

    def __init__(self, waveforms, onsets, device=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        is_tensor = hasattr(waveforms, "data_ptr")
        if is_tensor or (isinstance(waveforms, np.ndarray) and waveforms.ndim == 3):
            if waveforms.ndim != 3 or waveforms.shape[1] != 3:
                raise ValueError(f"expected (N, 3, L) waveforms, got {tuple(waveforms.shape)}")
            lengths = np.full(waveforms.shape[0], waveforms.shape[2], np.int64)
        else:
            waveforms = [np.asarray(w) for w in waveforms]
            for i, w in enumerate(waveforms):
                if w.ndim != 2 or w.shape[0] != 3:
                    raise ValueError(f"trace {i}: expected a (3, L) array, got {w.shape}")
            lengths = np.array([w.shape[1] for w in waveforms], np.int64)
        n = len(lengths)
        if n == 0:
            raise ValueError("an empty waveform bank")
        self.n_traces = n
        self.lengths = lengths
        self.onsets = _onset_table(onsets, n)
        self.device = int(waveforms.device.index if is_tensor and waveforms.is_cuda else device)
        _lib.check(self._lib.vp_bank_create(self.device, n, int(3 * lengths.sum()), C.byref(self._h)), "vp_bank_create")
        if is_tensor:
            if not waveforms.is_cuda:
                waveforms = waveforms.numpy()
            else:
                t = waveforms.float().contiguous()
                self._write(0, n, C.c_void_p(t.data_ptr()), _lib.VP_MEM_DEVICE)
                return
        first = 0
        while first < n:  # chunks of whole traces
            last, floats = first, 0
            while last < n and (last == first or floats + 3 * lengths[last] <= self.CHUNK_FLOATS):
                floats += 3 * int(lengths[last])
                last += 1
            if isinstance(waveforms, np.ndarray):
                chunk = np.ascontiguousarray(waveforms[first:last], np.float32)
            else:
                chunk = np.concatenate([np.asarray(w, np.float32).ravel() for w in waveforms[first:last]])
            self._write(first, last - first, chunk.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST)
            first = last

    def _write(self, first, count, ptr, mem):
        lens = np.ascontiguousarray(self.lengths[first:first + count])
        ons = np.ascontiguousarray(self.onsets[first:first + count])
        _lib.check(self._lib.vp_bank_write(self._h, first, count, ptr, mem, lens.ctypes.data_as(C.POINTER(C.c_int64)),
                                           ons.ctypes.data_as(C.POINTER(C.c_double))), "vp_bank_write")

    @classmethod
    def from_metadata(cls, waveforms, metadata, phase_dict=PHASE_DICT, device=0):
        """Onsets from the reference's metadata columns (a DataFrame or a dict of arrays): every column of ``phase_dict``
        that ``metadata`` has, up to two per phase, in ``phase_dict``'s order."""
        n = len(waveforms)
        onsets = {}
        for col, phase in phase_dict.items():
            if col in metadata:
                onsets.setdefault(phase, []).append(np.asarray(metadata[col], np.float64).reshape(n))
        for phase, cols in onsets.items():
            if len(cols) > 2:
                raise ValueError(f"phase {phase!r}: {len(cols)} columns, the bank holds two per phase")
            onsets[phase] = np.stack(cols, axis=1)
        return cls(waveforms, onsets, device=device)

    def make_batch(self, rows, model, sigma):
        """``{"X", "y"}``: (B, 3, model.in_samples) fp32 CUDA tensors written on torch's current stream -- what
        ``PhaseNetLit.training_step`` / ``validation_step`` take."""
        import torch

        rows = as_rows(rows)
        T = int(model.in_samples)
        dev = torch.device("cuda", self.device)
        x = torch.empty((len(rows), 3, T), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        lr_ = label_rows(model.labels)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._lib.vp_bank_make_batch(self._h, rows.ctypes.data_as(C.c_void_p), len(rows), T, float(sigma),
                                                _norm(model.norm), lr_.ctypes.data_as(C.POINTER(C.c_int)),
                                                C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(stream)),
                   "vp_bank_make_batch")
        return {"X": x, "y": y}

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vp_bank_destroy(self._h)
            self._h = None

    __del__ = close


def _norm(norm):
    if norm not in ("peak", "std"):
        raise ValueError(f"norm must be 'peak' or 'std', got {norm!r}")
    return _lib.VP_NORM_PEAK if norm == "peak" else _lib.VP_NORM_STD


class WindowPlanner:
    """Block 1's window choice (steps 1-2 of the module docstring) as plan rows, with ``np.random.default_rng(seed)``.

    ``bank`` is anything with ``lengths`` (N,) and ``onsets`` (N, 4) (a :class:`WaveformBank`).  Per row: with
    probability ``first_window_prob[0] / sum(first_window_prob)`` the around-a-pick branch -- an onset ``o`` drawn
    uniformly among the trace's finite onsets, ``p0 = int(o - samples_before)``, extent ``[p0, p0 + first_windowlen)`` --
    else the null branch, ``p0 = 0``, extent ``[0, L)``.  Then RandomWindow inside the extent of length ``n1``:
    ``low = sample_boundaries[0] or 0``, ``high = sample_boundaries[1] or n1``; ``p1 = low`` when ``high - low < in_samples``
    (zero fill at the end), else uniform in ``[low, high - in_samples]``.  The row: ``start = p0 + p1``,
    ``lo = max(0, p0)``, ``hi = min(L, p0 + n1)``."""

    def __init__(self, bank, batch_size, samples_before=3000, first_windowlen=6000, first_window_prob=(2, 1),
                 sample_boundaries=(None, None), in_samples=3001, seed=0):
        self.lengths = np.asarray(bank.lengths, np.int64)
        self.onsets = np.asarray(bank.onsets, np.float64).reshape(len(self.lengths), 4)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        prob = np.asarray(first_window_prob, np.float64)
        if prob.shape != (2,) or (prob < 0).any() or prob.sum() <= 0:
            raise ValueError(f"first_window_prob: two non-negative weights, got {first_window_prob}")
        self.p_around = float(prob[0] / prob.sum())
        self.samples_before = samples_before
        self.first_windowlen = int(first_windowlen)
        self.low, self.high = sample_boundaries
        self.in_samples = int(in_samples)
        self.rng = np.random.default_rng(seed)

    def plan(self, traces) -> np.ndarray:
        """Plan rows for the given trace indices, in that order."""
        traces = np.asarray(traces, np.int64)
        n = len(traces)
        rng = self.rng
        L = self.lengths[traces]
        ons = self.onsets[traces]
        finite = np.isfinite(ons)
        n_on = finite.sum(axis=1)
        around = rng.random(n) < self.p_around
        k = rng.integers(0, np.maximum(n_on, 1))  # index among the trace's finite onsets
        if NO_PICK_FALLBACK == "error" and (around & (n_on == 0)).any():
            raise ValueError(f"trace {int(traces[around & (n_on == 0)][0])} has no pick for the around-a-pick branch")
        around &= n_on > 0
        # the k-th finite onset of each row (columns P, P, S, S)
        rank = np.cumsum(finite, axis=1) - 1
        pick = np.where(finite & (rank == k[:, None]), ons, 0.0).sum(axis=1)
        p0 = np.where(around, P0_ROUNDING(pick - self.samples_before), 0).astype(np.int64)
        if not PAD_LEFT_AT_NEGATIVE_P0:
            p0 = np.maximum(p0, 0)
        n1 = np.where(around, self.first_windowlen, L).astype(np.int64)
        low = np.full(n, self.low or 0, np.int64)
        high = np.full(n, self.high, np.int64) if self.high else n1
        span = high - low - self.in_samples + 1
        p1 = np.where(span >= 1, low + rng.integers(0, np.maximum(span, 1)), low)
        rows = np.zeros(n, PLAN_ROW)
        rows["trace"] = traces
        rows["start"] = p0 + p1
        rows["lo"] = np.maximum(0, p0)
        rows["hi"] = np.minimum(L, p0 + n1)
        return rows

    def epoch(self):
        """One training epoch: a new permutation of the traces in batches, the last partial batch dropped
        (the reference's training DataLoader: shuffle=True, drop_last=True)."""
        perm = self.rng.permutation(len(self.lengths))
        B = self.batch_size
        for i in range(0, len(perm) - B + 1, B):
            yield self.plan(perm[i:i + B])

    def validation(self):
        """The traces in order, the last partial batch kept (the reference's validation DataLoader)."""
        n, B = len(self.lengths), self.batch_size
        for i in range(0, n, B):
            yield self.plan(np.arange(i, min(i + B, n)))
