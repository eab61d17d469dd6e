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

With ``stack_data`` (every released config), the reference follows block 1 with volpick's stacking block
(``get_stack_block``, models.py:345-397), ``AddGap`` and a second ``Normalize`` (models.py:399-440, training and
validation alike).  :class:`AugmentedPlanner` plans these as well: one :data:`AUG_ROW` per window holds the primary plan
row, the truncation behind the first event, up to two stacked events (a source window or the window itself, where its
samples start, its shift and scale), up to two stacked noise windows, a Gaussian-noise factor with its counter-based
generator key, and the gap.  Everything that follows from onsets alone -- the first event's end, the sources' P-label
check, their label argmax, the shifts -- is computed on the host; the kernel (``vp_bank_make_batch_aug``,
``vp_train_step_bank_aug``) decides only what depends on sample values: the zero-channel rule, ``max|x|`` and
``max(x)``, the normalisation statistics and the combined labels.

SeisBench is not available to pin the generator semantics below; each choice that rests on its behaviour is one named
constant here:

* ``NO_PICK_FALLBACK`` -- what the around-a-pick branch does with a trace that has no finite onset;
* ``PAD_LEFT_AT_NEGATIVE_P0`` -- how a window that starts before the trace (``p0 < 0``) is filled;
* ``P0_ROUNDING`` -- how ``onset - samples_before`` becomes an integer sample;
* ``NOISE_RULE`` -- the noise label where the P and S Gaussians overlap;
* ``SELECTION_FIRST`` -- which onset ``WindowAroundSample(selection="first")`` centres on;
* ``GAUSSIAN_NOISE_SCALE`` -- what ``GaussianNoise`` scales its draw by;
* ``GAP_DRAW`` and ``GAP_NOISE_ROW`` -- how ``AddGap`` draws its gap and which label row it sets to 1 there;
* ``EVENT_END_INDEX`` -- how a non-integer first-event end becomes a sample index;
* ``STEERED_CENTRE``, ``STEERED_CLAMP`` and ``STEERED_SHORT_TRACE`` -- where ``SteeredWindow(strategy="pad")`` puts the
  window around its target (:class:`SteeredPlanner`, the evaluation windows of the pick-benchmark tasks 1-3);
* ``DETECTION_FACTOR``, ``DETECTION_ONSET``, ``DETECTION_INDEX``, ``DETECTION_NEEDS`` and ``DETECTION_ORDER`` -- the
  box ``DetectionLabeller`` draws from P to behind S (EQTransformer's ``detections`` row);
* ``DETECTION_UNSHIFTED`` -- what the stacked events do with the detection box of a source whose shift is 0.

EQTransformer's block 1 (``EQTransformerLit.get_joint_augmentation_block1``, models.py:606-666) differs in three things:
the windows (``samples_before=6000``, ``windowlen=12000``, ``RandomWindow(windowlen=6000)``), the labeller's
``noise_column=False`` -- ``y`` is the P and S rows alone, not rescaled -- and a ``DetectionLabeller`` that writes
``detections``.  ``vp_bank_make_batch_eqt`` executes it on the same plan rows; :meth:`WaveformBank.make_batch` chooses it
for a model whose labels start with ``"Detection"``.

EQTransformer's stacked recipe (``EQTransformerLit.get_train_augmentations`` / ``get_val_augmentations``, models.py:668-844)
is block 1, the stacking block, ``AddGap`` and a second ``Normalize`` as well.  :class:`AugmentedPlanner` plans it with
the model's windows -- the primary and the noise sources with the block 1 above, the event sources with
``samples_before=3000``, ``windowlen=8000`` (``event_samples_before`` / ``event_windowlen``;
``EQTransformerLit.augmented_planner`` sets them) -- and ``vp_bank_make_batch_eqt_aug``
(:meth:`WaveformBank.make_batch_eqt_aug`) executes the same :data:`AUG_ROW` records with three differences:

* ``noise_label=False``: behind an event ``y = max(y, y')`` and nothing else -- no division by ``max(1, P + S)``, no noise
  row;
* ``detection_keys=["detections"]``: a source carries its own detection box (``DetectionLabeller`` on the source window's
  onsets; for a duplicate the window's own box), shifted with zero fill and merged by maximum -- but the reference's shift
  has no branch for a shift of 0, so an unshifted source's box is dropped while its waveform and its P and S are merged
  (``DETECTION_UNSHIFTED``);
* ``AddGap(label_keys=["y", "detections"], noise_id={})``: in the gap x, P, S and the detection row are all 0, no row is 1.

Stacked noise leaves the labels alone and the second ``Normalize`` is PhaseNet's.  Everything the planner decides from
onsets alone carries over unchanged.

Out of scope: array rotation (``rotate_array`` defaults to False and no config sets it); EQTransformer training.
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
SELECTION_FIRST = "earliest"  # selection="first": the earliest finite onset of the four columns (no draw)
GAUSSIAN_NOISE_SCALE = "signed_max"  # GaussianNoise: x += U(0, 0.15) * max(x) * N(0, 1), the signed maximum, not max|x|
GAP_DRAW = "start_then_end"  # AddGap: gap_lo uniform in [0, T), then gap_hi uniform in [gap_lo, T)
GAP_NOISE_ROW = "model"     # AddGap: labels in the gap 0, the model's noise row (label_rows[2]) 1 -- SeisBench's noise_id
                            # default -1 is the last row, which is the noise row of volpick's PSN labels
EVENT_END_INDEX = np.trunc  # the first-event end e as a sample index: int(e), toward zero; x[:, min(T, int(e)):] = 0 then
                            # follows numpy slicing, a negative index counting from the end
STEERED_CENTRE = "floor"    # SteeredWindow: p0 = start - (windowlen - (end - start)) // 2 -- an odd remainder's extra sample
                            # lies behind the target
STEERED_CLAMP = True        # ... then p0 is moved into [0, L - windowlen]: a window inside the trace, not zeros beside it
STEERED_SHORT_TRACE = "pad_end"  # a trace shorter than windowlen: p0 = 0, zeros behind the trace, borders as given
# DetectionLabeller(p_phases, s_phases=s_phases), ndim == 2 (EQTransformer's block 1; fixed in the kernel, asserted where
# the rule is restated): y[p0:p1] = 1 with p0 = max(int(p), 0), p1 = max(int(s + DETECTION_FACTOR * (s - p)), 0)
DETECTION_FACTOR = 1.4      # the detection ends factor * (S - P) behind S; 0 with a fixed window, where s = p + fixed_window
DETECTION_ONSET = "earliest"  # p and s: the minimum of the phase's finite onsets (window-relative)
DETECTION_INDEX = np.trunc  # int(.): truncation toward zero, of p and of the end; the end rounds its product before its sum
DETECTION_NEEDS = "P and S"  # no finite P onset or no finite S onset: the row is 0
DETECTION_ORDER = "s >= p"  # an S before the P: the row is 0 (s == p with no tail: an empty slice)
# SuperimposeEvent / MyDuplicateEvent with detection_keys (EQTransformer's stacked recipe; fixed in the kernel): the shift of
# the source's detection row has a branch for a shift to the right and one for a shift to the left, none for a shift of 0
DETECTION_UNSHIFTED = "dropped"  # shifted_first_pick == original_first_pick: the source's detection row is not merged

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

# include/volpick_hip.h vp_assemble_piece: one source trace's contribution to one (trace, component) row of a bank
ASSEMBLE_PIECE = np.dtype([("src", np.uint64), ("mean_n", np.int64), ("keep_lo", np.int64), ("keep_n", np.int64),
                           ("dst", np.int64), ("trace", np.int32), ("component", np.int32), ("kind", np.int32),
                           ("reserved", np.int32)], align=True)
assert ASSEMBLE_PIECE.itemsize == C.sizeof(_lib.VpAssemblePiece)

AUG_NONE, AUG_BANK, AUG_SELF = _lib.VP_AUG_NONE, _lib.VP_AUG_BANK, _lib.VP_AUG_SELF
AUG_EVENT = np.dtype([("row", PLAN_ROW), ("kind", np.int32), ("zero_before", np.int32), ("shift", np.int32),
                      ("scale", np.float32)], align=True)
AUG_NOISE = np.dtype([("row", PLAN_ROW), ("kind", np.int32), ("scale", np.float32)], align=True)
# include/volpick_hip.h vp_aug_row: the primary plan row and what follows it (AugmentedPlanner); unused entries are zero
AUG_ROW = np.dtype([("primary", PLAN_ROW), ("event", AUG_EVENT, (2,)), ("noise", AUG_NOISE, (2,)), ("noise_key", np.uint64),
                    ("gauss", np.float32), ("cut", np.int32), ("gap_lo", np.int32), ("gap_hi", np.int32)], align=True)
assert AUG_ROW.itemsize == C.sizeof(_lib.VpAugRow)


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


def as_aug_rows(rows) -> np.ndarray:
    """A contiguous, non-empty 1-D AUG_ROW array."""
    rows = np.asarray(rows)
    if rows.dtype != AUG_ROW:
        raise TypeError("augmented rows must have the dtype generate.AUG_ROW")
    if rows.ndim != 1 or rows.size == 0:
        raise ValueError("augmented rows: a non-empty 1-D array")
    return np.ascontiguousarray(rows)


def label_rows(labels) -> np.ndarray:
    """Output row of P, S and noise for a model's ``labels`` (e.g. "PSN" or "NPS")."""
    labels = "".join(labels)
    if sorted(labels) != ["N", "P", "S"]:
        raise ValueError(f"labels must be a permutation of 'PSN', got {labels!r}")
    return np.array([labels.index("P"), labels.index("S"), labels.index("N")], np.int32)


def has_detection_row(labels) -> bool:
    """True for EQTransformer's labels (``["Detection", "P", "S"]``): the batch carries a detection row, not a noise row."""
    return "Detection" in list(labels)


def detection_label_rows(labels) -> np.ndarray:
    """Output row of detection, P and S for an EQTransformer's ``labels`` (``["Detection", "P", "S"]`` in any order)."""
    labels = list(labels)
    if sorted(labels) != ["Detection", "P", "S"]:
        raise ValueError(f"labels must be a permutation of ['Detection', 'P', 'S'], got {labels!r}")
    return np.array([labels.index("Detection"), labels.index("P"), labels.index("S")], np.int32)


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
    def from_pieces(cls, pieces, lengths, onsets, device=0, sources=()):
        """A bank assembled on the device from source arrays that already live there (``vp_bank_assemble``, one call for
        every trace): ``pieces`` is an :data:`ASSEMBLE_PIECE` array grouped by (trace, component), ``lengths`` the traces'
        lengths, ``onsets`` as for the constructor.  Runs on torch's current stream and does not wait for it.  ``sources``
        (the tensors the pieces point into) are kept alive with the bank."""
        import torch

        pieces = np.ascontiguousarray(pieces)
        if pieces.dtype != ASSEMBLE_PIECE or pieces.ndim != 1:
            raise TypeError("pieces: a 1-D array of generate.ASSEMBLE_PIECE")
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
        n = self.n_traces = len(self.lengths)
        if n == 0:
            raise ValueError("an empty waveform bank")
        self.onsets = _onset_table(onsets, n)
        self.device = int(device)
        self._sources = list(sources)
        _lib.check(self._lib.vp_bank_create(self.device, n, int(3 * self.lengths.sum()), C.byref(self._h)), "vp_bank_create")
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        _lib.check(self._lib.vp_bank_assemble(self._h, 0, n, pieces.ctypes.data_as(C.c_void_p), len(pieces),
                                              self.lengths.ctypes.data_as(C.POINTER(C.c_int64)),
                                              np.ascontiguousarray(self.onsets).ctypes.data_as(C.POINTER(C.c_double)),
                                              C.c_void_p(stream)), "vp_bank_assemble")
        return self

    def trace(self, i):
        """Trace ``i`` read back: its (3, L_i) float32 array on the host (``vp_bank_read``; waits for the device)."""
        i = int(i)
        if not 0 <= i < self.n_traces:
            raise IndexError(f"trace {i} outside [0, {self.n_traces})")
        out = np.empty((3, int(self.lengths[i])), np.float32)
        _lib.check(self._lib.vp_bank_read(self._h, i, out.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST), "vp_bank_read")
        return out

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

    def make_batch(self, rows, model, sigma, detection_fixed_window=None):
        """``{"X", "y"}``: (B, 3, model.in_samples) fp32 CUDA tensors written on torch's current stream -- what
        ``PhaseNetLit.training_step`` / ``validation_step`` take.  ``rows``: plan rows (``PLAN_ROW``, block 1 alone) or
        augmented rows (``AUG_ROW``, from :class:`AugmentedPlanner`).

        A model with a detection row (an EQTransformer) gets ``{"X": (B, 3, T), "y": (B, 2, T), "detections": (B, 1, T)}``,
        what ``EQTransformerLit.shared_step`` reads: ``y`` holds P and S, and both are views of one (B, 3, T) tensor in the
        order detection, P, S (``vp_bank_make_batch_eqt``; plan rows only -- augmented rows go to
        :meth:`make_batch_eqt_aug`).  ``detection_fixed_window``: the detection's
        length in samples from P, ``None`` = to behind S (the module's ``DETECTION_*`` constants)."""
        aug = getattr(rows, "dtype", None) == AUG_ROW
        if has_detection_row(model.labels):
            if aug:
                raise ValueError("augmented rows with an EQTransformer model: make_batch executes block 1 alone for it; "
                                 "its stacked recipe is WaveformBank.make_batch_eqt_aug (EQTransformerLit.make_batch)")
        elif detection_fixed_window is not None:
            raise ValueError("detection_fixed_window: the model has no detection row")
        return self._make(rows, model, sigma, detection_fixed_window)

    def make_batch_eqt_aug(self, rows, model, sigma, detection_fixed_window=None):
        """EQTransformer's stacked recipe (``vp_bank_make_batch_eqt_aug``) on augmented rows (``AUG_ROW``, from
        ``EQTransformerLit.augmented_planner``): ``{"X": (B, 3, T), "y": (B, 2, T), "detections": (B, 1, T)}`` on torch's
        current stream, ``y`` and ``detections`` views of one (B, 3, T) tensor in the order detection, P, S, as
        :meth:`make_batch` returns them for plan rows.  ``model`` must have a detection row."""
        if not has_detection_row(model.labels):
            raise ValueError("make_batch_eqt_aug: the model has no detection row (make_batch takes its augmented rows)")
        detection_label_rows(model.labels)
        return self._make(as_aug_rows(rows), model, sigma, detection_fixed_window)

    def _make(self, rows, model, sigma, detection_fixed_window):
        """The batch of ``rows`` for ``model`` by one of the four ``vp_bank_make_batch*``: ``_aug`` for augmented rows,
        ``_eqt`` (with the detection window, the rows of y in the order detection, P, S) for a model with a detection row."""
        import torch

        aug = getattr(rows, "dtype", None) == AUG_ROW
        det = has_detection_row(model.labels)
        if det:
            detection_label_rows(model.labels)  # (the model's labels are what the batch is laid out for)
        rows = as_aug_rows(rows) if aug else as_rows(rows)
        name = "vp_bank_make_batch" + ("_eqt" if det else "") + ("_aug" if aug else "")
        if det:
            lr_, tail = np.array([0, 1, 2], np.int32), (_fixed_window(detection_fixed_window),)
        else:
            lr_, tail = label_rows(model.labels), ()
        dev = torch.device("cuda", self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        x = torch.empty((len(rows), 3, int(model.in_samples)), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        _lib.check(getattr(self._lib, name)(self._h, rows.ctypes.data_as(C.c_void_p), len(rows), int(model.in_samples),
                                            float(sigma), _norm(model.norm), lr_.ctypes.data_as(C.POINTER(C.c_int)), *tail,
                                            C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(stream)), name)
        return {"X": x, "y": y[:, 1:3], "detections": y[:, 0:1]} if det else {"X": x, "y": y}

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


def _fixed_window(detection_fixed_window):
    """The C argument det_fixed_window: the length in samples, or -1 for ``None`` (the detection follows S)."""
    if detection_fixed_window is None:
        return -1.0
    w = float(detection_fixed_window)
    if not (np.isfinite(w) and w >= 0):
        raise ValueError(f"detection_fixed_window must be None or a finite length >= 0, got {detection_fixed_window!r}")
    return w


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
                 sample_boundaries=(None, None), in_samples=3001, seed=0, selection="random"):
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
        if selection not in ("random", "first"):
            raise ValueError(f"selection must be 'random' or 'first', got {selection!r}")
        self.selection = selection
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
        if self.selection == "random":
            k = rng.integers(0, np.maximum(n_on, 1))  # index among the trace's finite onsets
        if NO_PICK_FALLBACK == "error" and (around & (n_on == 0)).any():
            raise ValueError(f"trace {int(traces[around & (n_on == 0)][0])} has no pick for the around-a-pick branch")
        around &= n_on > 0
        if self.selection == "random":  # the k-th finite onset of each row (columns P, P, S, S)
            rank = np.cumsum(finite, axis=1) - 1
            pick = np.where(finite & (rank == k[:, None]), ons, 0.0).sum(axis=1)
        else:
            assert SELECTION_FIRST == "earliest"
            pick = np.where(finite, ons, np.inf).min(axis=1)
            pick = np.where(n_on > 0, pick, 0.0)
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


class SteeredPlanner:
    """``SteeredWindow(windowlen=in_samples, strategy="pad")`` as plan rows: the evaluation windows of the pick-benchmark
    tasks 1-3 (the reference's ``get_eval_augmentations``, driven by the task targets' ``start_sample`` / ``end_sample``).

    ``bank`` is anything with ``lengths`` (N,).  Per target ``(trace, start, end)`` with ``w = end - start``:
    ``p0 = start - (in_samples - w) // 2``, moved into ``[0, L - in_samples]``; a trace shorter than the window is taken
    from ``p0 = 0`` and zero-filled behind its end.  The row is ``(trace, start=p0, lo=0, hi=L)`` and the window border
    ``(start - p0, end - p0)``: the target's samples, local to the window.  ``ValueError`` for a target longer than the
    window, one that is empty or starts before the trace, and one whose end no window can hold (past the trace's end, or
    past ``in_samples`` on a short trace)."""

    def __init__(self, bank, in_samples):
        self.lengths = np.asarray(bank.lengths, np.int64)
        self.in_samples = int(in_samples)
        if self.in_samples < 1:
            raise ValueError("in_samples must be >= 1")

    def plan(self, targets):
        """``(rows, window_borders)``: a PLAN_ROW array and an (n, 2) int32 array, in the targets' order.  ``targets``: a
        DataFrame or a dict of arrays with ``trace`` (bank index), ``start_sample`` and ``end_sample``."""
        assert STEERED_CENTRE == "floor" and STEERED_CLAMP and STEERED_SHORT_TRACE == "pad_end"
        trace = np.asarray(targets["trace"], np.int64)
        start = np.asarray(targets["start_sample"])
        end = np.asarray(targets["end_sample"])
        if (start != np.floor(start)).any() or (end != np.floor(end)).any():
            raise ValueError("start_sample / end_sample must be whole samples (resampled targets are out of scope)")
        start, end = start.astype(np.int64), end.astype(np.int64)
        if ((trace < 0) | (trace >= len(self.lengths))).any():
            raise ValueError(f"target traces outside [0, {len(self.lengths)})")
        T = self.in_samples
        L = self.lengths[trace]
        w = end - start
        if (w > T).any():
            i = int(np.flatnonzero(w > T)[0])
            raise ValueError(f"target {i}: [{start[i]}, {end[i]}) is longer than the window of {T} samples")
        if ((w < 1) | (start < 0)).any():
            i = int(np.flatnonzero((w < 1) | (start < 0))[0])
            raise ValueError(f"target {i}: [{start[i]}, {end[i]}) is empty or starts before the trace")
        p0 = np.clip(start - (T - w) // 2, 0, np.maximum(L - T, 0))
        if (end - p0 > T).any():
            i = int(np.flatnonzero(end - p0 > T)[0])
            raise ValueError(f"target {i}: [{start[i]}, {end[i]}) ends behind every window of trace {trace[i]} ({L[i]} samples)")
        rows = np.zeros(len(trace), PLAN_ROW)
        rows["trace"] = trace
        rows["start"] = p0
        rows["hi"] = L
        borders = np.stack([start - p0, end - p0], axis=1).astype(np.int32)
        return rows, borders


def trace_subsets(metadata, column="source_type", noise_value="noise"):
    """``(event_traces, noise_traces)``: the bank indices whose ``metadata[column]`` is not / is ``noise_value`` -- the
    reference's split of a set into the stacked-event and stacked-noise generators (its train.py filters on
    ``source_type``)."""
    col = np.asarray(metadata[column]).astype(str)
    noise = col == noise_value
    return np.flatnonzero(~noise), np.flatnonzero(noise)


class Augmentation:
    """The reference's stacking block, gap and second Normalize (models.py:345-440) with its defaults, and the trace
    subsets they draw from: ``event_traces`` / ``noise_traces`` index the training bank, ``val_event_traces`` /
    ``val_noise_traces`` the validation bank (``trace_subsets`` builds them from a ``source_type`` column).  An empty or
    ``None`` subset switches its slot off, as a missing generator does in the reference."""

    def __init__(self, event_traces=None, noise_traces=None, val_event_traces=None, val_noise_traces=None,
                 event_prob=(0.2, 0.2, 0.6), noise_prob=(0.25, 0.25, 0.5), gap_prob=(0.2, 0.8), event_inv_scale=(0.25, 4),
                 noise_inv_scale=(2, 50), gauss_scale=(0, 0.15), sep=200, tail_length_factor=1.4,
                 prob_num_events=None):
        self.event_traces, self.noise_traces = event_traces, noise_traces
        self.val_event_traces, self.val_noise_traces = val_event_traces, val_noise_traces
        self.params = dict(event_prob=event_prob, noise_prob=noise_prob, gap_prob=gap_prob, event_inv_scale=event_inv_scale,
                           noise_inv_scale=noise_inv_scale, gauss_scale=gauss_scale, sep=sep,
                           tail_length_factor=tail_length_factor, prob_num_events=prob_num_events)

    def planner(self, bank, batch_size, seed, in_samples=3001, sigma=20, validation=False, event_samples_before=1500,
                event_windowlen=4000, **block1):
        ev, nz = (self.val_event_traces, self.val_noise_traces) if validation else (self.event_traces, self.noise_traces)
        return AugmentedPlanner(bank, batch_size, ev, nz, seed=seed, in_samples=in_samples, sigma=sigma,
                                event_samples_before=event_samples_before, event_windowlen=event_windowlen, **self.params,
                                **block1)


# columns of AugmentedPlanner's uniform draws, one row per window (AugmentedPlanner.last_draws["u"])
U_COLS = {"event_branch": 0, "n_events": 1, "event_source": (2, 3), "event_q": (4, 5), "event_scale": (6, 7),
          "noise_branch": 8, "n_noise": 9, "noise_source": (10, 11), "noise_scale": (12, 13), "gauss": 14, "gap_branch": 15,
          "gap_lo": 16, "gap_hi": 17}
N_U = 18
P_CHECK_TOL = 1e-2 + 1e-5  # np.isclose(max P, 1, atol=1e-2): |max P - 1| <= atol + rtol * 1


def _int_draw(u, lo, hi):
    """The integer lo + floor(u (hi - lo)) in [lo, hi) for a uniform u in [0, 1) (hi > lo)."""
    return lo + np.minimum(np.floor(u * (hi - lo)).astype(np.int64), hi - lo - 1)


def _slice_start(k, T):
    """numpy's start index of x[:, k:] for an int k (negative: counted from the end)."""
    return np.where(k >= 0, np.minimum(k, T), np.maximum(T + k, 0))


def _phase_peak(o, lo, hi, two_s2):
    """The peak of the label row max_j exp(-(s - o_j)^2 / two_s2) over integer samples s in [lo, hi), in float64: o (n, 2)
    onsets (NaN = none) in the row's samples.  Returns (value, argmax); value 0 (argmax lo) for an empty range, no onset or
    a row that is 0 everywhere.  Ties go to the lowest sample, as np.argmax: the best sample of each onset is its floor or
    ceiling clamped into the range, so the row's maximum is at one of those four candidates."""
    n = len(o)
    hi1 = np.maximum(hi - 1, lo)
    fin = np.isfinite(o)
    fl = np.floor(np.where(fin, o, 0.0))
    cand = np.concatenate([fl, fl + 1], axis=1)  # (n, 4)
    cand = np.minimum(np.maximum(cand, lo[:, None]), hi1[:, None])
    d = np.where(fin[:, None, :], cand[:, :, None] - np.where(fin, o, 0.0)[:, None, :], np.inf)  # (n, 4 cand., 2 onsets)
    g = np.exp(-(d * d) / two_s2).max(axis=2)
    g = np.where((hi > lo)[:, None], g, 0.0)
    val = g.max(axis=1)
    arg = np.where(g == val[:, None], cand, np.inf).min(axis=1)
    arg = np.where(val > 0, arg, lo).astype(np.int64)
    return val, arg.reshape(n)


def _shifted_argmax(o, d, T, two_s2):
    """np.argmax over t in [0, T) of a label row shifted by d with zero fill: row(t) = peak row(t - d) for 0 <= t - d < T."""
    val, arg = _phase_peak(o, np.maximum(0, -d), np.minimum(T, T - d), two_s2)
    return np.where(val > 0, arg + d, 0)


class AugmentedPlanner:
    """Block 1 followed by the reference's stacking slots, AddGap and second Normalize (models.py:399-440) as
    :data:`AUG_ROW` records, with the ``plan`` / ``epoch`` / ``validation`` surface of :class:`WindowPlanner`.

    The primary rows come from ``WindowPlanner(bank, batch_size, seed=seed, ...)`` itself, so they equal its rows batch
    for batch; everything else is drawn from a second generator seeded from ``seed``.  ``event_traces`` /
    ``noise_traces`` are index subsets of ``bank``; an empty or ``None`` subset switches its slot off.  Event sources are
    planned as the reference's stacked-event generator does (block 1 with ``samples_before=event_samples_before``,
    ``windowlen=event_windowlen``, ``selection="first"``, probabilities ``[1, 0]``: 1500 / 4000 for PhaseNet, 3000 / 8000
    for EQTransformer), noise sources with the primary's block 1 (``**block1``: ``samples_before``, ``first_windowlen``,
    ...; PhaseNet's defaults when empty).  ``sigma`` must be the label width the batches are made with: the sources'
    P-label check and label argmax depend on it.

    Per window, in order (``u`` = the window's uniforms, columns :data:`U_COLS`): the event slot ``OneOf([superimpose,
    duplicate, null], event_prob)``, the noise slot ``OneOf([superimpose noise, Gaussian noise, null], noise_prob)``, the
    gap ``OneOf([AddGap, null], gap_prob)``.  An integer in ``[lo, hi)`` is ``lo + floor(u (hi - lo))``, a scale
    ``1 / (a + u (b - a))`` for ``inv_scale = (a, b)``, a source ``subset[floor(u len(subset))]``.  ``last_draws`` holds
    the latest batch's draws (``u``, the source traces and rows, the noise keys) for a replay."""

    def __init__(self, bank, batch_size, event_traces=None, noise_traces=None, seed=0, in_samples=3001, sigma=20,
                 event_prob=(0.2, 0.2, 0.6), noise_prob=(0.25, 0.25, 0.5), gap_prob=(0.2, 0.8), event_inv_scale=(0.25, 4),
                 noise_inv_scale=(2, 50), gauss_scale=(0, 0.15), sep=200, tail_length_factor=1.4, prob_num_events=None,
                 event_samples_before=1500, event_windowlen=4000, **block1):
        self.primary = WindowPlanner(bank, batch_size, in_samples=in_samples, seed=seed, **block1)
        self.lengths, self.onsets = self.primary.lengths, self.primary.onsets
        self.batch_size, self.T = self.primary.batch_size, int(in_samples)
        self.rng = np.random.default_rng([int(seed), 0x5354_4143_4B])  # the augmentation draws' own stream
        n = len(self.lengths)

        def subset(ix):
            ix = np.asarray([] if ix is None else ix, np.int64).ravel()
            if ((ix < 0) | (ix >= n)).any():
                raise ValueError(f"trace subset: indices outside [0, {n})")
            return ix

        self.event_traces, self.noise_traces = subset(event_traces), subset(noise_traces)

        def probs(p, k):
            p = np.asarray(p, np.float64)
            if p.shape != (k,) or (p < 0).any() or p.sum() <= 0:
                raise ValueError(f"branch probabilities: {k} non-negative weights, got {p}")
            return np.cumsum(p / p.sum())

        self.event_cum, self.noise_cum, self.gap_cum = probs(event_prob, 3), probs(noise_prob, 3), probs(gap_prob, 2)
        pne = {1: 0.7, 2: 0.3} if prob_num_events is None else dict(prob_num_events)
        if not set(pne) <= {1, 2}:
            raise ValueError(f"prob_num_events: at most two events per window, got {sorted(pne)}")
        self.num_choices = np.array(list(pne), np.int64)
        self.num_cum = probs(list(pne.values()), len(pne))
        self.event_inv_scale, self.noise_inv_scale = event_inv_scale, noise_inv_scale
        self.gauss_scale = gauss_scale
        self.sep, self.tail = int(sep), float(tail_length_factor)
        self.two_s2 = 2.0 * float(sigma) ** 2
        # the sources' block 1 (models.py:274-280; EQTransformer's :679-682), drawing from the augmentation stream
        self.event_planner = WindowPlanner(bank, batch_size, samples_before=event_samples_before,
                                           first_windowlen=event_windowlen, first_window_prob=(1, 0), in_samples=in_samples,
                                           selection="first")
        self.noise_planner = WindowPlanner(bank, batch_size, in_samples=in_samples, **block1)
        self.event_planner.rng = self.noise_planner.rng = self.rng
        self.last_draws = None

    def _sources(self, subset, u, need, planner):
        """Source traces (n, 2) drawn from subset with the uniforms u (n, 2), and their block-1 rows for the windows
        `need` (zero elsewhere)."""
        n = len(u)
        tr, rows = np.zeros((n, 2), np.int64), np.zeros((n, 2), PLAN_ROW)
        if len(subset):
            tr = subset[_int_draw(u, 0, len(subset))]
            k = np.flatnonzero(need)
            if len(k):
                rows[k] = planner.plan(tr[k].ravel()).reshape(len(k), 2)
        return tr, rows

    def _onsets(self, trace, start):
        """Window-local onsets (n, 4) of rows of `trace` starting at `start`."""
        return self.onsets[trace] - start[:, None].astype(np.float64)

    def plan(self, traces) -> np.ndarray:
        """Augmented rows for the given trace indices, in that order."""
        prim = self.primary.plan(traces)
        n, T, sep = len(prim), self.T, self.sep
        rng = self.rng
        u = rng.random((n, N_U))
        ev_branch = np.searchsorted(self.event_cum, u[:, U_COLS["event_branch"]], side="right")
        nz_branch = np.searchsorted(self.noise_cum, u[:, U_COLS["noise_branch"]], side="right")
        ev_tr, ev_rows = self._sources(self.event_traces, u[:, list(U_COLS["event_source"])], ev_branch == 0,
                                       self.event_planner)
        nz_tr, nz_rows = self._sources(self.noise_traces, u[:, list(U_COLS["noise_source"])], nz_branch == 0,
                                       self.noise_planner)
        keys = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
        self.last_draws = {"u": u, "event_traces": ev_tr, "event_rows": ev_rows, "noise_traces": nz_tr,
                           "noise_rows": nz_rows, "noise_key": keys}

        out = np.zeros(n, AUG_ROW)
        out["primary"] = prim
        out["cut"] = T

        # --- event slot: worked out on the windows that draw superimpose or duplicate only -------------------------
        if len(self.event_traces):
            ix = np.flatnonzero(ev_branch < 2)
            self._events(out, ix, ev_branch[ix] == 0, u[ix], ev_rows[ix])

        # --- noise slot -------------------------------------------------------------------------------------------
        if len(self.noise_traces):
            n_nz = self.num_choices[np.searchsorted(self.num_cum, u[:, U_COLS["n_noise"]], side="right")]
            a0, a1 = self.noise_inv_scale
            for j in range(2):
                on = np.flatnonzero((nz_branch == 0) & (j < n_nz))
                nz = out["noise"][:, j]
                nz["kind"][on] = AUG_BANK
                nz["row"][on] = nz_rows[on, j]
                nz["scale"][on] = 1.0 / (a0 + u[on, U_COLS["noise_scale"][j]] * (a1 - a0))
            g0, g1 = self.gauss_scale
            assert GAUSSIAN_NOISE_SCALE == "signed_max"  # applied in the kernel
            gauss = np.where(nz_branch == 1, (g0 + u[:, U_COLS["gauss"]] * (g1 - g0)).astype(np.float32), 0.0)
            out["gauss"] = gauss
            out["noise_key"] = np.where(out["gauss"] > 0, keys, 0)

        # --- gap ----------------------------------------------------------------------------------------------------
        assert GAP_DRAW == "start_then_end" and GAP_NOISE_ROW == "model"
        gap = np.searchsorted(self.gap_cum, u[:, U_COLS["gap_branch"]], side="right") == 0
        glo = _int_draw(u[:, U_COLS["gap_lo"]], 0, T)
        ghi = _int_draw(u[:, U_COLS["gap_hi"]], glo, T)
        out["gap_lo"] = np.where(gap, glo, 0)
        out["gap_hi"] = np.where(gap, ghi, 0)
        return out

    def _events(self, out, ix, sup, u, ev_rows):
        """The event slot of windows ix (sup: superimpose, else duplicate) into out."""
        n, T, sep = len(ix), self.T, self.sep
        prim = out["primary"][ix]
        n_ev = self.num_choices[np.searchsorted(self.num_cum, u[:, U_COLS["n_events"]], side="right")]
        ons = self._onsets(prim["trace"], prim["start"])
        fin = np.isfinite(ons)
        n_on = fin.sum(axis=1)
        mx = np.where(fin, ons, -np.inf).max(axis=1)
        mn = np.where(fin, ons, np.inf).min(axis=1)
        with np.errstate(invalid="ignore"):
            e_many = EVENT_END_INDEX(mx + np.maximum((mx - mn) * self.tail, sep) + 0.2 * sep)
            e_one = mx + 1 + sep
        # SuperimposeEvent casts the one-onset end to int, MyDuplicateEvent does not
        e = np.where(n_on >= 2, e_many, np.where(sup, EVENT_END_INDEX(e_one), e_one))
        # P-label peaks of the window itself and of both sources, in one pass
        src = [np.where(sup[:, None], self._onsets(ev_rows[:, i]["trace"], ev_rows[:, i]["start"]), ons) for i in range(2)]
        val, arg = _phase_peak(np.concatenate([ons[:, 0:2], src[0][:, 0:2], src[1][:, 0:2]]), np.zeros(3 * n, np.int64),
                               np.full(3 * n, T, np.int64), self.two_s2)
        pv, pa = val[:n], arg[:n]
        active = (n_on > 0) & (sup | (np.abs(pv - 1.0) <= P_CHECK_TOL))
        e = np.where(active, e, 0.0)
        out["cut"][ix] = np.where(active, _slice_start(EVENT_END_INDEX(e).astype(np.int64), T), T)
        stopped = ~active
        events = out["event"][ix]
        for i in range(2):
            alive = ~stopped & (i < n_ev)
            stop = np.where(sup, e >= T - 2 * sep, e + 2 * sep >= T)
            stopped |= alive & stop
            alive &= ~stop
            # the source: its window (superimpose) or the window itself (duplicate)
            so = src[i]
            sv, sa = val[(i + 1) * n:(i + 2) * n], arg[(i + 1) * n:(i + 2) * n]
            a = np.where(sup, sa, pa)
            added = alive & (~sup | (np.abs(sv - 1.0) <= P_CHECK_TOL))
            lo = EVENT_END_INDEX(e).astype(np.int64)
            hi = np.where(sup, T - 2 * sep, T - sep)
            q = _int_draw(u[:, U_COLS["event_q"][i]], lo, np.maximum(hi, lo + 1))
            d = np.clip(q - a, -T, T)  # |d| = T: wholly outside the window, as any |d| >= T
            a0, a1 = self.event_inv_scale
            ev = events[:, i]
            k = np.flatnonzero(added)
            ev["kind"][k] = np.where(sup[k], AUG_BANK, AUG_SELF)
            ks = np.flatnonzero(added & sup)
            ev["row"][ks] = ev_rows[ks, i]
            ev["zero_before"][k] = np.maximum(a[k] - sep, 0)
            ev["shift"][k] = d[k]
            ev["scale"][k] = 1.0 / (a0 + u[k, U_COLS["event_scale"][i]] * (a1 - a0))
            if i == 0:  # the next event starts behind this one's latest label peak
                k = np.flatnonzero(added & (n_ev > 1))
                dk = np.concatenate([d[k], d[k]])
                am = _shifted_argmax(np.concatenate([so[k, 0:2], so[k, 2:4]]), dk, T, self.two_s2)
                e[k] = np.maximum(e[k], np.maximum(am[:len(k)], am[len(k):]) + 1 + sep)
        out["event"][ix] = events

    def epoch(self):
        """As WindowPlanner.epoch (the primary planner's permutation), each batch augmented."""
        for rows in self.primary.epoch():
            yield self._augment(rows)

    def validation(self):
        """As WindowPlanner.validation, each batch augmented (the reference's get_val_augmentations)."""
        for rows in self.primary.validation():
            yield self._augment(rows)

    def _augment(self, rows):
        # plan() for traces whose primary rows are already drawn: replay them through a one-shot primary
        saved = self.primary.plan
        self.primary.plan = lambda traces: rows
        try:
            return self.plan(rows["trace"])
        finally:
            self.primary.plan = saved
