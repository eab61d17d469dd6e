"""Picker API of the volpick path on MI355X: ``PhaseNet`` / ``EQTransformer`` with the
``seisbench.models`` surface volpick users call.

Reference usage this mirrors (names, argument meaning, error behaviour):
  README.md:46-66            from_pretrained("volpick"); classify(stream, batch_size=256, overlap=5500,
                             blinding=(500,500), stacking="avg", parallelism=None, P_threshold=..,
                             S_threshold=.., copy=True).picks
  Final_models/demo.ipynb    list_pretrained() (:60,92), .weights_docstring (:121), .device/.cuda()
                             (:224-227), annotate(stream, overlap=, blinding=) -> traces
                             "<Model>_<label>" (:300-327), classify(...).picks (:397-413)
  volpick/model/eval_taks0.py:58-89   model.eval(); model(x) on (B,3,T) float32 tensors;
                             model.name / model.labels / model.device
  model_training/test.ipynb:231-240   .labels .norm .component_order .default_args

Every numerical stage runs in libvolpick_hip.so (HIP, gfx950) through ctypes; torch is only
used for device buffers and tensors handed back to the caller.  There is no CPU path: using a
model without a GPU / without the built library raises ``VolpickHipError``.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import time
import warnings
from pathlib import Path

import numpy as np

from . import _lib
from ._device import device_backing
from ._lib import VolpickHipError
from .picks import ClassifyOutput, Detection, DetectionList, Pick, PickList
from .stream import Stream, Trace, UTCDateTime, block_dict, block_start, plan_blocks, warn_short_fragment

WEIGHTS_DIR = Path(__file__).resolve().parent / "weights"


def _torch():
    import torch

    return torch


def OrderedDictTensors(arrays, torch):
    from collections import OrderedDict

    return OrderedDict((k, torch.from_numpy(np.array(v, order="C"))) for k, v in arrays.items())


# Triggers are five COLUMNS everywhere inside the package: (spec index, on, off, peak, value), numpy int32, int64 x 3, float32.
_TRIGGER_DTYPES = (np.int32, np.int64, np.int64, np.int64, np.float32)
_I32P, _I64P, _F32P = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)


def _trigger_columns(found=()):
    """[(spec, on, off, peak, value)] or the five columns -> the five columns (nothing: five empty ones)."""
    if isinstance(found, tuple) and found:
        return found
    z = list(zip(*found)) or [()] * 5
    return tuple(np.asarray(c, dt) for c, dt in zip(z, _TRIGGER_DTYPES))


def _trigger_tuples(cols):
    """The five columns -> [(spec, on, off, peak, value)] of Python numbers: the form bench.py, the tools and some tests read."""
    return list(zip(*(c.tolist() for c in cols)))


class _TriggerBuffer:
    """Result arrays of one trigger scan with room for ``cap`` triggers (``with_block``: and vp_classify_multi's block index)."""

    def __init__(self, cap, with_block=False):
        self.cap = int(cap)
        self._cols = tuple(np.empty(self.cap, dt) for dt in _TRIGGER_DTYPES)
        self.block_of = np.empty(self.cap, np.int32) if with_block else None
        self.found = C.c_int()

    def pointers(self):
        """on, off, peak, value, spec_of[, block_of], as vp_pick_rows / vp_classify_collect / vp_classify_multi order them."""
        spec_of, on, off, peak, val = self._cols
        p = [on.ctypes.data_as(_I64P), off.ctypes.data_as(_I64P), peak.ctypes.data_as(_I64P), val.ctypes.data_as(_F32P),
             spec_of.ctypes.data_as(_I32P)]
        return p if self.block_of is None else p + [self.block_of.ctypes.data_as(_I32P)]

    def columns(self):
        """The ``found`` triggers as columns of their own (the ``cap``-sized arrays are not kept alive by them)."""
        m = self.found.value
        return tuple(c[:m].copy() for c in self._cols)


def _records_from_columns(cols, tids, t0s, labels, sr):
    """Trigger columns of all station blocks -> (PickList, DetectionList), sorted as the records sort ((start_time,
    trace_id, phase) / (start_time, trace_id), stable), the records deferred.  Times: t0 + k / sr in integer microseconds,
    rounded as stream.UTCDateTime.__add__ rounds (float64 k / sr * 1e6, half to even)."""
    if not cols:
        return PickList(), DetectionList()
    grp = np.concatenate([np.full(len(c[1]), c[0], np.int64) for c in cols])
    spec, on, off, peak, val = (np.concatenate([c[i] for c in cols]) for i in range(1, 6))
    t0 = np.asarray(t0s, np.int64)[grp]
    us = lambda k: t0 + np.rint(k / float(sr) * 1e6).astype(np.int64)
    start, end, top = us(on), us(off), us(peak)
    order = {t: i for i, t in enumerate(sorted(set(tids)))}  # equal ids (two blocks of one station) compare equal
    tid_rank = np.asarray([order[t] for t in tids], np.int64)[grp]
    lab_rank = np.asarray([sorted(set(labels)).index(l) for l in labels], np.int64)[spec] if labels else spec
    is_det = np.asarray([l == "Detection" for l in labels], bool)[spec]
    U = UTCDateTime._from_us

    def build(mask, keys, make_one):
        idx = np.flatnonzero(mask)
        idx = idx[np.lexsort(tuple(k[idx] for k in keys))]
        g, s_, a, b, c, v = grp[idx].tolist(), spec[idx].tolist(), start[idx].tolist(), end[idx].tolist(), top[idx].tolist(), val[idx].tolist()
        return len(idx), (lambda: [make_one(tids[g[i]], a[i], b[i], c[i], v[i], labels[s_[i]]) for i in range(len(g))])

    n_p, make_p = build(~is_det, (lab_rank, tid_rank, start), lambda tid, a, b, c, v, ph: Pick(tid, U(a), U(b), U(c), v, ph))
    n_d, make_d = build(is_det, (tid_rank, start), lambda tid, a, b, c, v, ph: Detection(tid, U(a), U(b), v))
    return PickList._deferred(n_p, make_p), DetectionList._deferred(n_d, make_d)


class WaveformModel:
    """Common host logic: weight registry, device handle, stream handling, annotate/classify."""

    name = "WaveformModel"
    _kind = -1
    _weights_subdir = ""
    in_samples = 0
    default_contexts = 3
    sampling_rate = 100.0
    # class-level annotate defaults (SeisBench ``_annotate_args``), overridden by the JSON's default_args
    _annotate_args = {
        "batch_size": 256,
        "overlap": 0,
        "stacking": "avg",
        "blinding": (0, 0),
        "*_threshold": 0.3,
    }
    _known_args = {"batch_size", "overlap", "stacking", "blinding", "parallelism", "copy", "strict",
                   "flexible_horizontal_components", "stride"}

    def __init__(self, component_order="ZNE", norm="peak", filter_args=None, filter_kwargs=None, **kwargs):
        self.component_order = component_order
        self.norm = norm
        # SeisBench: ``trace.filter(*filter_args, **filter_kwargs)`` on every trace inside annotate() / classify()
        self.filter_args = tuple(filter_args) if filter_args is not None else None
        self.filter_kwargs = dict(filter_kwargs) if filter_kwargs is not None else None
        self.default_args = {}
        self.weights_docstring = None
        self._weights_metadata = None
        self._weights_version = None
        self._weights = None  # flat fp32 blob in the library's canonical order
        self._handle = None
        self._extra_handles = []
        self.batch_across_blocks = True  # classify(): windows of several device-resident blocks share the forward batches
        self._max_windows_per_call = 32768  # bounds the prediction buffer of one multi-block call (2.4 GB for EQT)
        # device contexts classify() pipelines station blocks over (PhaseNet 3, EQTransformer 4; more contexts than that
        # only add queueing)
        self.n_contexts = self.default_contexts
        self._seg_per_context = 2  # segments of a long block per device context (<= VP_MAX_INFLIGHT submit slots)
        self._device_index = None
        self._max_batch = 256
        self._plan_flags = (0, 0)  # vp_config.plan_flags[0:2]: (layer-by-layer plan, dump fused intermediates)
        self._timing = None        # dict: classify() records its phases there, SERIALISED by device synchronisations (bench.py `api`)
        self._training = False
        if norm not in ("peak", "std"):
            raise ValueError("norm must be 'peak' or 'std'")

    # ------------------------------------------------------------------ weights
    @classmethod
    def list_pretrained(cls, details=False, remote=False):
        d = WEIGHTS_DIR / cls._weights_subdir
        names = sorted(p.stem for p in d.glob("*.json"))
        if details:
            return {n: json.loads((d / f"{n}.json").read_text()).get("docstring", "") for n in names}
        return names

    @classmethod
    def from_pretrained(cls, name, version_str="latest", update=False, force=False, wait_for_file=False):
        d = WEIGHTS_DIR / cls._weights_subdir
        meta_path, npz_path = d / f"{name}.json", d / f"{name}.npz"
        if not meta_path.exists() or not npz_path.exists():
            raise ValueError(f"No pretrained {cls.__name__} weights '{name}'. Available: {cls.list_pretrained()}")
        meta = json.loads(meta_path.read_text())
        with np.load(npz_path) as z:
            tensors = {k: z[k] for k in z.files}
        return cls._from_state(meta, tensors)

    @classmethod
    def load(cls, path, version_str=None):
        """Load SeisBench-format ``<path>.json[.vN]`` + ``<path>.pt[.vN]`` (torch state dict)."""
        path = str(path)
        suffix = f".v{version_str}" if version_str else ""
        meta = json.loads(Path(path + ".json" + suffix).read_text())
        sd = _torch().load(path + ".pt" + suffix, map_location="cpu", weights_only=True)
        return cls._from_state(meta, {k: v.numpy() for k, v in sd.items()})

    @classmethod
    def _from_state(cls, meta, tensors):
        model = cls(**meta.get("model_args", {}))
        model.load_state_dict(tensors)
        model.default_args = dict(meta.get("default_args", {}))
        model.weights_docstring = meta.get("docstring")
        model._weights_version = meta.get("version")
        model._weights_metadata = meta
        return model

    def load_state_dict(self, tensors, strict=True):
        lib = _lib.load()
        parts = []
        expected = set()
        for i in range(lib.vp_param_count(self._kind)):
            key = lib.vp_param_name(self._kind, i).decode()
            expected.add(key)
            if key not in tensors:
                raise KeyError(f"missing key in state dict: {key}")
            a = np.asarray(getattr(tensors[key], "numpy", lambda: tensors[key])(), dtype=np.float32).ravel()
            if a.size != lib.vp_param_size(self._kind, i):
                raise ValueError(f"size mismatch for {key}: {a.size} vs {lib.vp_param_size(self._kind, i)}")
            parts.append(a)
        extra = [k for k in tensors if k not in expected and not k.endswith("num_batches_tracked")]
        if strict and extra:
            raise KeyError(f"unexpected keys in state dict: {extra[:5]}")
        self._weights = np.ascontiguousarray(np.concatenate(parts))
        # key order / shapes / non-float buffers of the source dict, so state_dict() and save() round-trip it
        self._state_layout = [(k, tuple(np.shape(tensors[k])), k in expected) for k in tensors if k not in extra]
        self._state_buffers = {k: np.array(getattr(tensors[k], "numpy", lambda k=k: tensors[k])())
                               for k, _, is_param in self._state_layout if not is_param}
        self._release()

    def state_dict(self):
        """``OrderedDict`` name -> numpy array in the source dict's key order (torch layout and names)."""
        from collections import OrderedDict

        if self._weights is None:
            raise RuntimeError("no weights loaded")
        lib = _lib.load()
        offsets, off = {}, 0
        for i in range(lib.vp_param_count(self._kind)):
            n = lib.vp_param_size(self._kind, i)
            offsets[lib.vp_param_name(self._kind, i).decode()] = (off, n)
            off += n
        out = OrderedDict()
        for key, shape, is_param in self._state_layout:
            if is_param:
                o, n = offsets[key]
                out[key] = self._weights[o:o + n].reshape(shape).copy()
            else:
                out[key] = self._state_buffers[key].copy()
        return out

    def get_model_args(self):
        args = {"component_order": self.component_order, "norm": self.norm}
        if self.filter_args is not None or self.filter_kwargs is not None:  # absent from the JSON of a model without a filter
            args["filter_args"] = list(self.filter_args) if self.filter_args is not None else None
            args["filter_kwargs"] = self.filter_kwargs
        return args

    def _stream_filter(self):
        """(args, kwargs) of the filter annotate() / classify() apply to every trace, or None."""
        if self.filter_args is None and self.filter_kwargs is None:
            return None
        return self.filter_args or (), self.filter_kwargs or {}

    def save(self, path, weights_docstring="", version_str=None):
        """Write ``<path>.json[.vN]`` + ``<path>.pt[.vN]`` in the SeisBench model-zoo format
        (the files ``model_training/tune.ipynb`` cell 7 ``export_model`` produces and
        ``Final_models/*/*.{json,pt}.v1`` hold), so weights round-trip through ``load``."""
        torch = _torch()
        path = str(path)
        suffix = f".v{version_str}" if version_str else ""
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        meta = {
            "docstring": weights_docstring or self.weights_docstring or "",
            "model_args": self.get_model_args(),
            "seisbench_requirement": (self._weights_metadata or {}).get("seisbench_requirement", "0.4.0"),
            "version": str(version_str) if version_str else (self._weights_version or "1"),
            "default_args": dict(self.default_args),
        }
        Path(path + ".json" + suffix).write_text(json.dumps(meta, indent=4))
        torch.save(OrderedDictTensors(self.state_dict(), torch), path + ".pt" + suffix)

    # ------------------------------------------------------------------ device
    @property
    def device(self):
        torch = _torch()
        return torch.device("cpu") if self._device_index is None else torch.device("cuda", self._device_index)

    def cuda(self, device=None):
        torch = _torch()
        idx = torch.cuda.current_device() if device is None else torch.device(device if not isinstance(device, int) else f"cuda:{device}").index
        if idx is None:
            idx = torch.cuda.current_device()
        if idx != self._device_index:
            self._release()
            self._device_index = idx
        self._ensure_handle()
        return self

    def to(self, device):
        dev = _torch().device(device)
        if dev.type == "cpu":
            return self.cpu()
        return self.cuda(dev)

    def cpu(self):
        self._release()
        self._device_index = None
        return self

    def eval(self):
        self._training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("model objects run the inference path; the PhaseNet training step lives in "
                                      "volpick_amd.train (PhaseNetTrainer / PhaseNetLit)")
        return self.eval()

    def _config(self):
        lib = _lib.load()
        cfg = _lib.VpConfig()
        _lib.check(lib.vp_default_config(self._kind, C.byref(cfg)))
        cfg.norm = _lib.VP_NORM_PEAK if self.norm == "peak" else _lib.VP_NORM_STD
        cfg.max_batch = int(self._max_batch)
        flags = list(self._plan_flags)
        if os.environ.get("VOLPICK_PLAN_FLAGS"):  # A/B timing of plan variants through bench.py (debug): the entries the model
            env = [int(v) for v in os.environ["VOLPICK_PLAN_FLAGS"].split(",")]  # itself left at 0 come from the environment
            flags += [0] * (len(env) - len(flags))
            flags = [f if f != 0 or i >= len(env) else env[i] for i, f in enumerate(flags)]
        for i, v in enumerate(flags):
            cfg.plan_flags[i] = int(v)
        return cfg

    def _ensure_handle(self, weights_device_ptr=None):
        if self._handle is not None:
            return self._handle
        torch = _torch()
        _lib.load()
        if not torch.cuda.is_available():
            raise VolpickHipError("no HIP device visible: the volpick path runs on MI355X only (no CPU fallback)")
        if self._weights is None:
            raise VolpickHipError("model has no weights; use from_pretrained() or load_state_dict()")
        if self._device_index is None:
            self._device_index = int(os.environ.get("LOCAL_RANK", torch.cuda.current_device())) % torch.cuda.device_count()
        self._handle = self._create(weights_device_ptr)
        return self._handle

    def _create(self, weights_device_ptr=None):
        """vp_create -> a new device context (own HIP stream + workspace) from the host blob, or from a device copy of it."""
        cfg, h, on_device = self._config(), C.c_void_p(), weights_device_ptr is not None
        ptr = C.c_void_p(weights_device_ptr) if on_device else self._weights.ctypes.data_as(C.c_void_p)
        _lib.check(_lib.load().vp_create(self._device_index, self._kind, ptr, self._weights.size,
                                         _lib.VP_MEM_DEVICE if on_device else _lib.VP_MEM_HOST, C.byref(cfg), C.byref(h)), "vp_create")
        return h

    def _context(self, k):
        """k-th device context of this model (own HIP stream + workspace).  Context 0 is ``_handle``; further ones are created
        on first use.  ``classify`` spreads blocks over them: one's latency-bound stages overlap another's MFMA-bound ones."""
        self._ensure_handle()
        if k == 0:
            return self._handle
        while len(self._extra_handles) < k:
            self._extra_handles.append(self._create())
        return self._extra_handles[k - 1]

    def _release(self):
        for h in getattr(self, "_extra_handles", []):
            _lib.load().vp_destroy(h)
        self._extra_handles = []
        if getattr(self, "_handle", None) is not None:
            try:
                _lib.load().vp_destroy(self._handle)
            finally:
                self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ------------------------------------------------------------------ model(x)
    def _forward_raw(self, x, preprocess=False):
        """(B,3,T) float32 torch tensor / ndarray -> (B,n_out,T) tensor on the input's device."""
        torch = _torch()
        lib = _lib.load()
        h = self._ensure_handle()
        as_numpy = isinstance(x, np.ndarray)
        if as_numpy:
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if x.ndim != 3 or x.shape[1] != 3 or x.shape[2] != self.in_samples:
            raise ValueError(f"expected input of shape (B, 3, {self.in_samples}), got {tuple(x.shape)}")
        x = x.contiguous().float()
        B = x.shape[0]
        on_dev = x.is_cuda
        if on_dev and x.device.index != self._device_index:
            raise ValueError(f"input on {x.device} but model on {self.device}")
        y = torch.empty((B, 3, self.in_samples), dtype=torch.float32, device=x.device)
        if B == 0:
            return y
        if on_dev:
            torch.cuda.current_stream(x.device).synchronize()
        mem = _lib.VP_MEM_DEVICE if on_dev else _lib.VP_MEM_HOST
        _lib.check(lib.vp_forward(h, C.c_void_p(x.data_ptr()), mem, B, int(preprocess), C.c_void_p(y.data_ptr()), mem),
                   "vp_forward")
        return y.numpy() if as_numpy else y

    def __call__(self, x, logits=False):
        if logits:
            raise NotImplementedError("logits=True is not part of the inference path")
        return self._format_output(self._forward_raw(x))

    forward = __call__

    def _format_output(self, y):
        return y

    # ------------------------------------------------------------------ annotate / classify
    def _argdict(self, kwargs):
        for k in kwargs:
            if k not in self._known_args and not k.endswith("_threshold"):
                warnings.warn(f"Unknown argument '{k}' will be ignored.")
        args = dict(kwargs)
        for k in ("overlap", "blinding", "stacking", "batch_size"):
            if k not in args:
                args[k] = self.default_args.get(k, self._annotate_args[k])
        if isinstance(args["overlap"], float) and 0 <= args["overlap"] < 1:  # fraction of the window
            args["overlap"] = int(self.in_samples * args["overlap"])
        args["overlap"] = int(args["overlap"])
        if not 0 <= args["overlap"] < self.in_samples:
            raise ValueError(f"overlap must be in [0, {self.in_samples}), got {args['overlap']}")
        b = tuple(int(v) for v in args["blinding"])
        if len(b) != 2 or min(b) < 0 or b[0] + b[1] >= self.in_samples:
            raise ValueError(f"invalid blinding {args['blinding']}")
        args["blinding"] = b
        if args["stacking"] not in ("avg", "max"):
            raise ValueError(f"Stacking method {args['stacking']} unknown. Known methods are 'avg' and 'max'.")
        return args

    def _threshold(self, args, label):
        key = f"{label}_threshold"
        if key in args:
            return float(args[key])
        if key in self.default_args:
            return float(self.default_args[key])
        return float(self._annotate_args.get(key, self._annotate_args["*_threshold"]))

    def _call_args(self, args):
        """(overlap, blinding left, blinding right, stacking, batch), as vp_annotate / vp_classify_submit / _multi take them."""
        stacking = _lib.VP_STACK_AVG if args["stacking"] == "avg" else _lib.VP_STACK_MAX
        batch = max(1, min(int(args["batch_size"]), self._max_batch))
        return args["overlap"], args["blinding"][0], args["blinding"][1], stacking, batch

    @staticmethod
    def _c_specs(specs):
        """``_trigger_specs``' list as the library's array."""
        return (_lib.VpTriggerSpec * len(specs))(*[_lib.VpTriggerSpec(r, on, off) for r, _, on, off in specs])

    def _upload(self, data, lo=None, hi=None, with_rows=False):
        """A (3,N) block -- device tensor (assembled there by _group_stream), ``_Rows`` or ndarray -- or its samples [lo, hi)
        -> contiguous float32 device tensor x, complete on return (the library runs on streams of its own).  ``with_rows``:
        -> (x, y), y the (3, len) array for the library's stacked rows, allocated behind x and ahead of the wait."""
        torch = _torch()
        dev = torch.device("cuda", self._device_index)
        if torch.is_tensor(data):  # ([None:None] is the whole block)
            x = data[:, lo:hi].to(dev, torch.float32).contiguous()
        elif isinstance(data, _Rows):
            x = data.slice(lo, hi).upload(torch, dev)
        else:
            x = torch.from_numpy(np.ascontiguousarray(data[:, lo:hi], dtype=np.float32)).to(dev)
        y = torch.empty((3, x.shape[1]), dtype=torch.float32, device=dev) if with_rows else None
        torch.cuda.current_stream(dev).synchronize()
        return (x, y) if with_rows else x

    def _lap(self, key, t0):
        """Profiled mode (``_timing`` is a dict: bench.py's `api`): add the milliseconds since ``t0`` to ``_timing[key]`` ->
        the time now, where the next interval starts.  Without, nothing happens."""
        if self._timing is None:
            return t0
        now = time.perf_counter()
        self._timing[key] = self._timing.get(key, 0.0) + (now - t0) * 1e3
        return now

    def _annotate_block(self, data, args):
        """(3,N) float32 ndarray -> (device tensor (n_out,N) with NaN, first_valid, last_valid, n_windows)."""
        lib = _lib.load()
        h = self._ensure_handle()
        x, out = self._upload(data, with_rows=True)
        fv, lv, nw = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(lib.vp_annotate(h, C.c_void_p(x.data_ptr()), _lib.VP_MEM_DEVICE, data.shape[1], *self._call_args(args),
                                   C.c_void_p(out.data_ptr()), _lib.VP_MEM_DEVICE, C.byref(fv), C.byref(lv),
                                   C.byref(nw)), "vp_annotate")
        return out, fv.value, lv.value, nw.value

    def _annotate_data(self, data, args):
        """``_annotate_segments`` for a block worth splitting over the device contexts, ``_annotate_block`` otherwise."""
        return (self._annotate_segments if self._is_long(data.shape[1], args) else self._annotate_block)(data, args)

    # ---- one long block spread over the device contexts ---------------------------------------------
    def _is_long(self, n_samples, args):
        """Worth splitting: every context gets at least two full forward batches."""
        step = self.in_samples - int(args["overlap"])
        batch = self._call_args(args)[4]
        return self.n_contexts > 1 and (n_samples - self.in_samples) // step + 1 >= 2 * batch * self.n_contexts

    def _annotate_segments(self, data, args):
        """Like ``_annotate_block`` for a long (3,N) block: ``segments.plan_segments`` cuts it into one segment
        per device context; segment r+1 is uploaded while segment r computes, the stacked outputs are cut and
        joined on the device -- sample for sample the unsplit result (volpick_amd/segments.py)."""
        job = self._segments_submit(data, args, 0)
        return job if isinstance(job, tuple) else self._segments_collect(job)

    def _segments_submit(self, data, args, slot_base, seg_per_context=None):
        """First half of ``_annotate_segments``: upload and enqueue every segment (submit slots ``slot_base`` .. on each
        context) -> a job for ``_segments_collect``; a block too short for more than one segment comes back finished, as
        ``_annotate_block``'s tuple.  ``classify()`` uploads the NEXT station's segments between the two halves."""
        from .segments import plan_segments

        lib = _lib.load()
        n = data.shape[1]
        # _seg_per_context segments per device context (one submit slot each): the first upload, which nothing overlaps, is that
        # much shorter
        nc = self.n_contexts
        segs = plan_segments(n, self.in_samples, args["overlap"], args["blinding"], nc * (seg_per_context or self._seg_per_context))
        if len(segs) == 1:
            return self._annotate_block(data, args)
        call_args = self._call_args(args)
        upload = lambda sg: self._upload(data, sg["lo"], sg["hi"], with_rows=True)  # noqa: E731

        def submit(r, sg, x, y):
            _lib.check(lib.vp_classify_submit(self._context(r % nc), slot_base + r // nc, C.c_void_p(x.data_ptr()), _lib.VP_MEM_DEVICE,
                                              sg["hi"] - sg["lo"], *call_args, None, 0, C.c_void_p(y.data_ptr()),
                                              _lib.VP_MEM_DEVICE, 0), "vp_classify_submit")

        jobs = []
        t0 = time.perf_counter()
        if self._timing is None:  # segment r + 1 is uploaded while segment r computes
            for r, sg in enumerate(segs):
                x, y = upload(sg)
                submit(r, sg, x, y)
                jobs.append((x, y))
        else:  # profiled: all uploads, then all compute (the two phases separated; their sum exceeds the pipelined wall time)
            jobs = [upload(sg) for sg in segs]
            t0 = self._lap("h2d_ms", t0)
            for r, (sg, (x, y)) in enumerate(zip(segs, jobs)):
                submit(r, sg, x, y)
        return dict(segs=segs, jobs=jobs, slot_base=slot_base, n=n, t0=t0, overlap=args["overlap"])

    def _segments_collect(self, job):
        """Second half: wait for the segments, cut and join their stacked outputs on the device."""
        torch = _torch()
        lib = _lib.load()
        dev = torch.device("cuda", self._device_index)
        nc, n, segs = self.n_contexts, job["n"], job["segs"]
        out = torch.empty((3, n), dtype=torch.float32, device=dev)
        fv = lv = -1
        found = C.c_int()
        for r, (sg, (x, y)) in enumerate(zip(segs, job["jobs"])):
            f, l, w = C.c_int64(), C.c_int64(), C.c_int64()
            _lib.check(lib.vp_classify_collect(self._context(r % nc), job["slot_base"] + r // nc, C.byref(f), C.byref(l), C.byref(w), None, None, None,
                                               None, None, 0, C.byref(found)), "vp_classify_collect")
            out[:, sg["keep_lo"]:sg["keep_hi"]] = y[:, sg["keep_lo"] - sg["lo"]:sg["keep_hi"] - sg["lo"]]
            if r == 0:
                fv = f.value
            lv = l.value + sg["lo"]
        n_windows = int(lib.vp_window_starts(n, self.in_samples, job["overlap"], None, 0))
        torch.cuda.current_stream(dev).synchronize()
        if self._timing is not None:
            self._lap("gpu_ms", job["t0"])
            self._timing["windows"] = self._timing.get("windows", 0) + n_windows
        return out, fv, lv, n_windows

    def _pick_rows(self, dev_out, specs, cap=8192, columns=False):
        """Trigger scan of the rows of a device (n_out, N) array -> [(spec_index, on, off, peak, value)]
        (``columns=True``: the same as five arrays)."""
        lib = _lib.load()
        h = self._ensure_handle()
        if not specs:
            return _trigger_columns() if columns else []
        dev_out = dev_out.contiguous()  # (a column slice of the stacked rows is a strided view)
        self._torch_sync(dev_out)
        c_specs = self._c_specs(specs)
        while True:  # every row in one launch, one synchronisation, one result copy
            buf = _TriggerBuffer(cap)
            _lib.check(lib.vp_pick_rows(h, C.c_void_p(dev_out.data_ptr()), dev_out.shape[1], c_specs, len(specs), *buf.pointers(), cap,
                                        C.byref(buf.found)), "vp_pick_rows")
            if buf.found.value <= cap:
                break
            cap = buf.found.value
        cols = buf.columns()  # grouped by spec, sorted by onset inside each group
        return cols if columns else _trigger_tuples(cols)

    @staticmethod
    def _torch_sync(t):
        """The library scans on its own stream: what torch has queued for this tensor must be done first."""
        _torch().cuda.current_stream(t.device).synchronize()

    def _trigger_specs(self, args):
        """[(row, label, thr_on, thr_off)]: picks use thr/thr, detections thr/(thr/2); 'N' is skipped."""
        specs = []
        for i, label in enumerate(self.labels):
            if label == "N":
                continue
            if label == "Detection":
                thr = self._threshold(args, "detection")
                specs.append((i, label, thr, thr / 2))
            else:
                thr = self._threshold(args, label)
                specs.append((i, label, thr, thr))
        return specs

    def _submit_block(self, ctx, data, args, specs, cap):
        """Enqueue one (3,N) block on device context ``ctx`` (no host synchronisation)."""
        lib = _lib.load()
        h = self._context(ctx)
        x = self._upload(data)
        _lib.check(lib.vp_classify_submit(h, 0, C.c_void_p(x.data_ptr()), _lib.VP_MEM_DEVICE, data.shape[1], *self._call_args(args),
                                          self._c_specs(specs), len(specs), None, _lib.VP_MEM_DEVICE, cap), "vp_classify_submit")
        return {"ctx": ctx, "x": x, "cap": cap, "data": data}  # x must outlive the submit

    def _collect_block(self, job, args, specs, columns=False):
        """Wait for a submitted block -> ([(spec_index, on, off, peak, value)], n_windows)
        (``columns=True``: the triggers as five arrays)."""
        lib = _lib.load()
        h = self._context(job["ctx"])
        buf = _TriggerBuffer(job["cap"])
        fv, lv, nw = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(lib.vp_classify_collect(h, 0, C.byref(fv), C.byref(lv), C.byref(nw), *buf.pointers(), buf.cap,
                                           C.byref(buf.found)), "vp_classify_collect")
        if buf.found.value > buf.cap:  # rare: more triggers than the result block holds -> redo this block with room
            job2 = self._submit_block(job["ctx"], job["data"], args, specs, buf.found.value)
            return self._collect_block(job2, args, specs, columns)
        cols = buf.columns()
        return (cols if columns else _trigger_tuples(cols)), nw.value

    def _classify_blocks(self, groups, args, specs, cap_per_row=256, columns=False):
        """Blocks of several stations in ONE library call -> one trigger list per block (``columns=True``: five arrays each)."""
        torch = _torch()
        lib = _lib.load()
        h = self._context(0)
        dev = torch.device("cuda", self._device_index)
        K = len(groups)
        lens = np.array([g["data"].shape[1] for g in groups], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(3 * lens)[:-1]]).astype(np.int64)
        # The one upload that is not ``_upload``: the blocks travel as ONE flat array, joined on the device when all of them
        # are there (classify()'s case), on the host otherwise.
        if all(torch.is_tensor(g["data"]) for g in groups):
            flat = torch.cat([g["data"].to(dev, torch.float32).reshape(-1) for g in groups])
        else:
            host = np.concatenate([(g["data"].cpu().numpy() if torch.is_tensor(g["data"]) else
                                    np.asarray(g["data"], dtype=np.float32)).reshape(-1) for g in groups])
            flat = torch.from_numpy(host).to(dev)
        torch.cuda.current_stream(dev).synchronize()
        c_specs, call_args = self._c_specs(specs), self._call_args(args)
        while True:
            cap = K * max(1, len(specs)) * cap_per_row
            buf = _TriggerBuffer(cap, with_block=True)
            _lib.check(lib.vp_classify_multi(
                h, C.c_void_p(flat.data_ptr()), _lib.VP_MEM_DEVICE, offsets.ctypes.data_as(_I64P), lens.ctypes.data_as(_I64P), K,
                *call_args, c_specs, len(specs), None, _lib.VP_MEM_DEVICE, None, None, None, *buf.pointers(), cap_per_row,
                cap, C.byref(buf.found)), "vp_classify_multi")
            if buf.found.value <= cap:
                break
            cap_per_row *= 8  # rare: some row holds more triggers than its slot list
        cols, block_of = buf.columns(), buf.block_of[:buf.found.value]
        out = [tuple(c[block_of == k] for c in cols) for k in range(K)]
        return out if columns else [_trigger_tuples(c) for c in out]

    def _classify_block(self, data, args, specs, cap=8192):
        """(3,N) float32 ndarray -> ([(spec_index, on, off, peak, value)], n_windows); indices into the block."""
        return self._collect_block(self._submit_block(0, data, args, specs, cap), args, specs)

    def annotate(self, stream, copy=True, **kwargs):
        """Sliding-window probability traces, one per label, named ``<Model>_<label>``."""
        args = self._argdict(kwargs)
        out = Stream()
        for grp in _group_stream(stream, self.component_order, self.sampling_rate, copy, self.in_samples, self._stream_filter()):
            dev_out, fv, lv, nw = self._annotate_data(grp["data"], args)
            if nw == 0 or fv < 0:
                continue
            host = dev_out[:, fv : lv + 1].cpu().numpy()
            for i, label in enumerate(self.labels):
                out.append(_make_trace(host[i], grp, fv, self.sampling_rate, f"{self.__class__.__name__}_{label}"))
        return _maybe_obspy(out, stream)

    def classify(self, stream, copy=True, **kwargs):
        """``annotate`` + trigger/peak extraction -> ``ClassifyOutput`` with ``.picks`` (and ``.detections``).  Every station
        block takes one of the three routes of ``_ClassifyRun``."""
        args = self._argdict(kwargs)
        specs = self._trigger_specs(args)
        return self._classify_groups(_group_stream(stream, self.component_order, self.sampling_rate, copy, self.in_samples,
                                                   self._stream_filter()), args, specs)

    def _classify_groups(self, groups, args, specs):
        """The station blocks ``groups`` (an iterator of ``block_dict``s: ``_group_stream``'s, or ``classify_files``' decoded
        ones) through the routes of one ``_ClassifyRun``, then the records."""
        torch = _torch()
        run = _ClassifyRun(self, args, specs)
        for grp in groups:
            if self._is_long(grp["data"].shape[1], args):
                run.add_long(grp)
            elif self.batch_across_blocks and torch.is_tensor(grp["data"]):
                run.add_resident(grp)
            else:
                run.add_host(grp)
        run.drain_long()
        run.drain_host()
        run.drain_resident()
        t_mark = time.perf_counter()
        picks, detections = _records_from_columns(run.cols, run.tids, run.t0s, [sp[1] for sp in specs], self.sampling_rate)
        self._lap("emit_records_ms", t_mark)
        return ClassifyOutput(self.name, picks=picks, detections=detections)

    def classify_files(self, sources, depth=2, workers=2, **kwargs):
        """``[self.classify(volpick_amd.read(s, device_resident=True), **kwargs) for s in sources]`` -- the same picks and
        detections, bit for bit -- with the host work and the upload of the files ahead running beside the classification of
        the one in flight (volpick_amd/files.py).  ``sources``: paths, bytes or file objects, as ``read`` takes them."""
        from .files import classify_files

        return classify_files(self, sources, depth=depth, workers=workers, **kwargs)


class _ClassifyRun:
    """One classify() call: the station blocks on their way through the device and the triggers back so far.  A block takes
    one of three routes, each an ``add_*`` (issue its work) and a ``drain_*`` (wait, scan, emit).  The ORDER in which they
    issue uploads, submits and collects is the optimisation (tests/test_gpu_classify_calls.py pins it).  The short routes
    use submit slot 0 of the contexts the long route fills: each drains the long route first, the long route the host route,
    and a resident chunk the host route before it goes.

    Triggers stay COLUMNS (numpy) from the library's result arrays to the sorted record lists: times in integer
    microseconds, one stable lexsort by Pick / Detection order (start time, trace id, phase), and the records themselves
    are built when the caller first touches the list (picks._PrintableList._deferred)."""

    def __init__(self, model, args, specs):
        self.model, self.args, self.specs = model, args, specs
        self.cols, self.tids, self.t0s = [], [], []  # (group index, spec indices, on, off, peak, value) per emitted block
        self.long_pending, self.n_long = [], 0       # [(block, job)] submitted, not collected; long blocks so far
        self.chunk, self.chunk_windows = [], 0       # resident blocks waiting for their common call; their windows
        self.host_pending, self.n_host = [], 0       # [(block, job)], oldest first; host blocks so far
        self.t_mark = time.perf_counter()            # profiled mode: where the host assembly of the next long block began

    def emit(self, grp, columns):
        if len(columns[0]):
            self.cols.append((len(self.tids),) + columns)
            self.tids.append(grp["trace_id"])
            self.t0s.append(grp["starttime"]._us)

    # ---- long: a day-long block; its segments occupy all contexts (``_segments_submit``)
    def add_long(self, grp):
        m, profiled = self.model, self.model._timing is not None
        self.drain_host()
        if profiled:  # the phases apart, one block at a time
            self.drain_long()
            m._lap("host_assembly_ms", self.t_mark)
        # Many stations: block k + 1 is uploaded and enqueued (on the other pair of submit slots) BEFORE block k is
        # collected, scanned and emitted -- the host's upload, the longest part of a PhaseNet station-day, then runs
        # beside block k's last segments instead of behind them.
        two_sets = 2 * m._seg_per_context <= _lib.VP_MAX_INFLIGHT  # a second set of submit slots for the block behind
        if not two_sets:
            self.drain_long()
        # (a block that is uploaded beside another one's compute goes as ONE segment per context: fewer, larger copies --
        # 2.82 -> 2.59 ms per station-day of eight; the first block of a call keeps the finer cut, whose first upload,
        # which nothing overlaps, is shorter: 3.09 vs 3.32 ms for a single station)
        job = m._segments_submit(grp["data"], self.args, m._seg_per_context * (self.n_long & 1) if two_sets else 0,
                                 1 if (two_sets and self.long_pending) else None)
        self.n_long += 1
        self.drain_long()
        self.long_pending.append((grp, job))
        if profiled:  # ... and finished at once
            self.drain_long()
            self.t_mark = time.perf_counter()

    def drain_long(self):
        while self.long_pending:
            grp, job = self.long_pending.pop(0)
            dev_out = job[0] if isinstance(job, tuple) else self.model._segments_collect(job)[0]
            t = time.perf_counter()
            found = self.model._pick_rows(dev_out, self.specs, columns=True)
            t = self.model._lap("pick_scan_d2h_ms", t)
            self.emit(grp, found)
            self.model._lap("emit_records_ms", t)

    # ---- resident: short blocks already on the device (read(..., device_resident=True)) are classified several at a time:
    # their windows share the forward batches (SeisBench's batch_size spans the whole stream) and stacking / trigger scan
    # are one launch per chunk of blocks, a chunk bounded by ``_max_windows_per_call``
    def add_resident(self, grp):
        m = self.model
        self.drain_long()
        n_windows = (grp["data"].shape[1] - m.in_samples) // (m.in_samples - int(self.args["overlap"])) + 2
        if self.chunk and self.chunk_windows + n_windows > m._max_windows_per_call:
            self.drain_resident()
        self.chunk.append(grp)
        self.chunk_windows += n_windows

    def drain_resident(self):
        m = self.model
        if self.chunk:  # a chunk that fills up in mid-stream finds host blocks in flight on context 0, whose slots it needs
            self.drain_host()
        if len(self.chunk) == 1:
            self._collect(self.chunk[0], m._submit_block(0, self.chunk[0]["data"], self.args, self.specs, 8192))
        elif self.chunk:
            for grp, columns in zip(self.chunk, m._classify_blocks(self.chunk, self.args, self.specs, columns=True)):
                self.emit(grp, columns)
        self.chunk, self.chunk_windows = [], 0

    # ---- host: short host blocks are pipelined one by one, round-robin over the device contexts, instead -- block i+1 is
    # assembled and enqueued while block i runs -- because for them the host-side assembly and copy, not the GPU, set the
    # pace (measured: 64 stations x 10 min, 8 ms of host assembly against 2.5 ms of GPU work)
    def add_host(self, grp):
        contexts = max(1, self.model.n_contexts)
        self.drain_long()
        if len(self.host_pending) == contexts:
            self._collect(*self.host_pending.pop(0))
        job = self.model._submit_block(self.n_host % contexts, grp["data"], self.args, self.specs, 8192)
        self.host_pending.append((grp, job))
        self.n_host += 1  # host blocks only: resident blocks must not advance the context

    def drain_host(self):
        while self.host_pending:
            self._collect(*self.host_pending.pop(0))

    def _collect(self, grp, job):
        self.emit(grp, self.model._collect_block(job, self.args, self.specs, True)[0])


class PhaseNet(WaveformModel):
    name = "PhaseNet"
    _kind = _lib.VP_MODEL_PHASENET
    _weights_subdir = "phasenet"
    in_samples = 3001
    _annotate_args = dict(WaveformModel._annotate_args, overlap=1500, blinding=(0, 0))
    _annotate_args["*_threshold"] = 0.3

    def __init__(self, in_channels=3, classes=3, phases="NPS", sampling_rate=100, norm="std", **kwargs):
        if in_channels != 3 or classes != 3 or len(phases) != 3:
            raise ValueError("only the released 3-component, 3-class PhaseNet topology is implemented")
        if sampling_rate != 100:
            raise ValueError("only 100 Hz models are implemented")
        super().__init__(norm=norm, **kwargs)
        self.labels = phases
        self.in_channels, self.classes = in_channels, classes

    def get_model_args(self):
        return dict(super().get_model_args(), phases=self.labels)


class EQTransformer(WaveformModel):
    name = "EQTransformer"
    _kind = _lib.VP_MODEL_EQTRANSFORMER
    _weights_subdir = "eqtransformer"
    in_samples = 6000
    default_contexts = 4
    _annotate_args = dict(WaveformModel._annotate_args, overlap=1800, blinding=(500, 500))
    _annotate_args["*_threshold"] = 0.1
    _annotate_args["detection_threshold"] = 0.3

    def __init__(self, in_channels=3, in_samples=6000, classes=2, phases="PS", sampling_rate=100, norm="std",
                 norm_amp_per_comp=False, **kwargs):
        if in_channels != 3 or in_samples != 6000 or classes != 2 or len(phases) != 2:
            raise ValueError("only the released 3-component, 6000-sample, P/S EQTransformer topology is implemented")
        if kwargs.pop("original_compatible", False):
            raise ValueError("original_compatible variants are not part of the volpick path")
        kwargs.pop("lstm_blocks", None), kwargs.pop("drop_rate", None)
        super().__init__(norm=norm, **kwargs)
        self.phases = phases
        self.labels = ["Detection"] + list(phases)
        self.norm_amp_per_comp = bool(norm_amp_per_comp)

    def get_model_args(self):
        args = dict(super().get_model_args(), phases=self.phases)
        if self.norm_amp_per_comp:
            args["norm_amp_per_comp"] = True
        return args

    def _config(self):
        cfg = super()._config()
        cfg.norm_amp_per_comp = int(self.norm_amp_per_comp)
        return cfg

    def _format_output(self, y):
        return tuple(y[:, i] for i in range(3))  # (detection, P, S), each (B, T)


class _Rows:
    """The (C, N) block of one instrument as its C full-length host rows, NOT yet stacked: the upload copies each
    row straight into the device array (for a day-long stream the host-side ``np.stack`` alone costs ~12 ms)."""

    def __init__(self, parts):
        self.parts = parts
        self.shape = (len(parts), len(parts[0]))

    def __array__(self, dtype=None, copy=None):
        a = np.stack(self.parts).astype(np.float32, copy=False)
        return a if dtype is None else a.astype(dtype, copy=False)

    def __getitem__(self, idx):
        return np.asarray(self)[idx]

    def slice(self, lo, hi):
        """Samples [lo, hi) of every row: views of the rows, nothing stacked."""
        return _Rows([p[lo:hi] for p in self.parts])

    def upload(self, torch, dev):
        """-> the device array.  Allocations and copies all go to the current stream and the staging temporaries live until
        this returns: torch's caching allocator hands their blocks out again only to work queued behind the copies."""
        x = torch.empty(self.shape, dtype=torch.float32, device=dev)
        hosts = [torch.from_numpy(np.ascontiguousarray(p)) for p in self.parts]
        # int32 counts (what a miniSEED file decodes to) and float64 rows travel as they are and are cast on the device: the
        # host-side cast of a day-long row costs 20 ms, 30 x its upload.  Rows in page-locked memory
        # (volpick_amd.pinned_array) go by DMA without the runtime's staging copy.
        temps = [None if h.dtype == torch.float32 else torch.empty(h.shape, dtype=h.dtype, device=dev) for h in hosts]
        for c, (h, t) in enumerate(zip(hosts, temps)):
            pinned = h.is_pinned()
            if t is None:
                x[c].copy_(h, non_blocking=pinned)
            else:
                t.copy_(h, non_blocking=pinned)
                x[c].copy_(t)
        return x


# --------------------------------------------------------------------------- stream handling
# SeisBench's annotate() runs annotate_stream_pre -- the model's filter -- ahead of its resampling: every trace is filtered at
# its OWN rate, then brought to the model's.
FILTER_BEFORE_RESAMPLE = True


def _prepare_trace(tr, sampling_rate, copy, stream_filter):
    """One trace of the caller's stream as the grouping takes it: filtered (if the model has a filter) and at the model's rate.
    With ``copy`` the caller's trace is never modified; without, it is processed in place, as upstream does."""
    from .resample import resample_trace

    def filt(t, may_modify):
        if stream_filter is None:
            return t
        from .signal import filtered_copy

        args, kwargs = stream_filter
        return t.filter(*args, **kwargs) if may_modify else filtered_copy(t, *args, **kwargs)

    if FILTER_BEFORE_RESAMPLE:
        out = filt(tr, not copy)
        return resample_trace(out, sampling_rate, copy and out is tr, fourier_on_device=True)
    out = resample_trace(tr, sampling_rate, copy, fourier_on_device=True)
    return filt(out, not copy or out is not tr)


def _group_stream(stream, component_order, sampling_rate, copy, in_samples, stream_filter=None):
    """Yield one dict per contiguous block of one instrument: data (3,N) float32 in
    ``component_order`` (missing components / gaps inside a block zero-filled), start time and
    ids.  In-repo twin of the array assembly: volpick/data/convert.py:26-70."""
    # traces at the model's rate are never modified, so ``copy`` needs no deep copy for them; the others are
    # resampled as SeisBench's annotate() does (on copies, or in place with copy=False); device-backed ones on the device,
    # whichever branch of the rule they take
    traces = [_prepare_trace(tr, float(sampling_rate), copy, stream_filter) for tr in stream]
    pieces = [(tr.stats.network, tr.stats.station, tr.stats.location, tr.stats.channel, UTCDateTime(tr.stats.starttime),
               int(tr.stats.npts) if device_backing(tr) is not None else len(tr.data), tr) for tr in traces]
    # which samples form a block is ``plan_blocks``' rule; here a block gets its samples, and only when it is reached
    for run in plan_blocks(pieces, component_order, sampling_rate, in_samples):
        if run.short:
            warn_short_fragment()
            continue
        b0, b1, used = run.b0, run.b1, run.used  # pieces: (first sample, length, component row or -1, trace)
        on_device = bool(used) and all(device_backing(p[3]) is not None for p in used)
        # the common case -- one full-length trace per component -- is a single stack, no zero fill
        full = sorted((p for p in used if p[0] == b0 and p[1] == b1 - b0), key=lambda p: p[2])
        if len(used) != len(component_order) or [p[2] for p in full] != list(range(len(component_order))):
            data = _zero_filled(run.pieces, b0, b1, len(component_order), used[0][3]._dev.device if on_device else None)
        elif on_device:
            data = _torch().stack([p[3]._dev for p in full]).float()
        else:
            data = _Rows([p[3].data.filled(0) if np.ma.isMaskedArray(p[3].data) else p[3].data for p in full])
        yield block_dict(data, run.network, run.station, run.location, block_start(run.t_start, b0, sampling_rate))


def _zero_filled(pieces, b0, b1, n_components, device):
    """Samples [b0, b1) of an instrument's ``pieces`` as one (C, b1 - b0) float32 array, zero where no trace has samples;
    on ``device`` when the traces were decoded on the GPU (read(..., device_resident=True)): assembled there, no host copy."""
    shape = (n_components, b1 - b0)
    data = np.zeros(shape, np.float32) if device is None else _torch().zeros(shape, dtype=_torch().float32, device=device)
    for s0, l, c, tr in sorted(pieces, key=lambda p: p[1]):  # shorter first: longer traces win overlaps
        lo, hi = max(s0, b0), min(s0 + l, b1)
        if c < 0 or hi <= lo:
            continue
        d = tr._dev[lo - s0 : hi - s0] if device is not None else tr.data[lo - s0 : hi - s0]
        data[c, lo - b0 : hi - b0] = d.filled(0) if np.ma.isMaskedArray(d) else d  # casts int / float64 counts to float32
    return data


def _make_trace(data, grp, first_valid, sampling_rate, channel):
    return Trace(data, {
        "network": grp["network"], "station": grp["station"], "location": grp["location"], "channel": channel,
        "starttime": grp["starttime"] + first_valid / sampling_rate, "sampling_rate": sampling_rate,
    })


def _maybe_obspy(out, like):
    """Return an obspy.Stream when the caller passed one (and obspy is importable)."""
    if type(like).__module__.startswith("obspy"):
        try:
            import obspy
        except ImportError:
            return out
        st = obspy.Stream()
        for tr in out:
            hdr = dict(tr.stats)
            hdr["starttime"] = obspy.UTCDateTime(tr.stats.starttime.timestamp)
            hdr.pop("npts", None)
            st.append(obspy.Trace(tr.data, hdr))
        return st
    return out
