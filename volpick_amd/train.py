"""PhaseNet training step on the GPU (BASELINE config 5).

Host-side mirror of the pieces of the reference's Lightning module that define the arithmetic of
one optimisation step (the reference's volpick/model/models.py):

* ``vector_cross_entropy`` (:34-51),
* ``PhaseNetLit.shared_step`` / ``training_step`` (:160-169): ``loss(model(batch["X"]), batch["y"])``,
* ``configure_optimizers`` (:177-185): ``torch.optim.Adam(lr)``,
* ``optimizer_step`` (:168-175): linear learning-rate warm-up over the first 500 steps.

Batches come either finished, as ``(x, y)`` tensors (``PhaseNetTrainer.step``, ``PhaseNetLit.training_step``), or are
generated on the GPU from a device-resident :class:`~volpick_amd.generate.WaveformBank`: window cut, demean and
normalise and Gaussian labels -- the core of the reference's augmentation block 1, its random choices planned on the
host by :class:`~volpick_amd.generate.WindowPlanner` (``PhaseNetTrainer.step_bank``, ``PhaseNetLit.fit_bank``).
Logging and checkpoint files (Lightning) are not part of this package.  Forward (training-mode BatchNorm), loss, backward and
Adam all run in ``libvolpick_hip.so`` (``vp_train_*``); there is no CPU fallback.

The validation half of the loop runs there too: ``validate_batches`` / ``PhaseNetLit.validate_bank`` generate each validation
batch from a bank, run the inference forward and reduce ``vector_cross_entropy`` in float64 on the GPU
(``vp_validate_begin`` / ``_bank`` / ``_end``), and ``fit_bank`` feeds that loss to what the released config trains with
(``configure_optimizers``, :187-219, and the callbacks of the reference's train.py:137-179): ``ReduceLROnPlateau`` (torch's
arithmetic, restated here without torch), the weights of the lowest validation loss, and the early stop.

EQTransformer has the validation half alone (``EQTransformerLit``, models.py:483-879): block 1's batch with its detection
row from a bank, or the stacked recipe's (``augmented_planner``, ``vp_bank_make_batch_eqt_aug``), and ``shared_step``'s
weighted binary cross entropy (``bce_loss`` on the host, ``validate_batches_eqt`` / ``EQTransformerLit.validate_bank`` on the
GPU: ``vp_validate_eqt_begin`` / ``_bank`` / ``_bank_aug`` / ``_end``).

EQTransformer's training step exists for the three decoder stacks and their heads with the trunk frozen
(``EQTransformerDecoderTrainer``, ``EQTransformerLit(trainable="decoders")``; ``vp_eqt_dec_train_*``): 48 tensors, 145,731 of
the model's trainable floats, fine-tuned from finished batches or from a bank through the same ``fit_bank`` host loop as
PhaseNet's.  Gradients into the trunk (pick LSTMs, attentions, transformers, BiLSTMs, ResCNN, encoder) are not implemented.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from .models import EQTransformer, PhaseNet


def vector_cross_entropy(y_pred, y_true, eps=1e-5):
    """models.py:34-51 on numpy arrays (B, C, T): mean over samples, sum over classes, mean over batch."""
    h = y_true * np.log(y_pred + eps)
    h = h.mean(-1).sum(-1) if y_pred.ndim == 3 else h.sum(-1)
    return -float(h.mean())


EQT_LOSS_WEIGHTS = (0.05, 0.40, 0.55)  # the reference's EQTransformerLit loss_weights: detection, P, S


def _loss_weights(loss_weights):
    """The three loss weights as the float64 array the library reads."""
    w = np.ascontiguousarray(loss_weights, np.float64)
    if w.shape != (3,):
        raise ValueError(f"loss_weights: three weights (detection, P, S), got {loss_weights!r}")
    return w


def bce_heads(p, y):
    """``torch.nn.BCELoss`` per window and row of (B, C, T) arrays, unreduced over both: the (B, C) float64 means over T
    of ``-(y max(log p, -100) + (1 - y) max(log(1 - p), -100))``.  The clamp is torch's and keeps a NaN."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        term = -(y * np.maximum(np.log(p), -100.0) + (1.0 - y) * np.maximum(np.log(1.0 - p), -100.0))
    return term.mean(-1)


def bce_loss(p, y, weights):
    """The loss of the reference's ``EQTransformerLit.shared_step`` (models.py:538-549) on numpy arrays (B, C, T):
    ``sum_c weights[c] * BCELoss(p[:, c], y[:, c])``, as the mean over the windows of ``sum_c weights[c] * head[b][c]``
    (every window has T samples, so the two are one number)."""
    w = np.asarray(weights, np.float64)
    heads = bce_heads(p, y)
    if w.shape != (heads.shape[1],):
        raise ValueError(f"weights: one per row, {heads.shape[1]}, got {w.shape}")
    return float((heads * w).sum(-1).mean())


def gaussian_labels(p_samples, s_samples, n_samples=3001, sigma=20.0):
    """Soft labels in ``phases = "PSN"`` order: Gaussians of width sigma at the P and S picks,
    noise = 1 - P - S (SeisBench ProbabilisticLabeller as PhaseNetLit configures it, models.py:254-260).
    NaN / negative picks leave the phase row zero."""
    B = len(p_samples)
    t = np.arange(n_samples, dtype=np.float64)
    y = np.zeros((B, 3, n_samples), dtype=np.float64)
    for row, picks in ((0, p_samples), (1, s_samples)):
        for b, s in enumerate(picks):
            if s is not None and np.isfinite(s) and s >= 0:
                y[b, row] = np.exp(-((t - float(s)) ** 2) / (2.0 * sigma ** 2))
    y[:, 2] = np.clip(1.0 - y[:, 0] - y[:, 1], 0.0, 1.0)
    return y.astype(np.float32)


class _Trainer:
    """What the two trainers share, over the entry points ``<_prefix>_*`` of the library: the handle with its hyper-parameters,
    the checks of a step's x / y, and the flat blob of ``names`` = ``[(tensor, size)]`` read and written by name."""

    _prefix = _model_type = _wrong_model = None  # "vp_train" / "vp_eqt_dec_train", the model's class, the refusal of another

    def __init__(self, model, max_batch, names, hyper, create):
        """``create(lib, weights, byref(handle))`` calls the library's constructor; ``hyper``: what follows the handle in
        ``<_prefix>_set_hyper``."""
        self._lib = _lib.load()
        self.model = model
        self.max_batch = int(max_batch)
        self.in_samples = model.in_samples
        self.names = names
        self.n_params = sum(n for _, n in names)
        self._h = C.c_void_p()
        w = np.ascontiguousarray(model._weights, dtype=np.float32)
        _lib.check(create(self._lib, w, C.byref(self._h)), self._prefix + "_create")
        try:
            _lib.check(self._c("set_hyper")(self._h, *hyper), self._prefix + "_set_hyper")
        except Exception:
            self.close()  # the handle exists already: release it with the refusal
            raise
        self.global_step = 0

    @classmethod
    def _check_model(cls, model):
        if not isinstance(model, cls._model_type):
            raise TypeError(cls._wrong_model)
        if model._weights is None:
            raise RuntimeError("model has no weights (use from_pretrained / load / load_state_dict)")

    def _c(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _arg(a):
        """(pointer, mem) of a numpy array or a CUDA torch tensor, fp32 contiguous."""
        if hasattr(a, "data_ptr"):
            if a.dtype != _torch().float32 or not a.is_contiguous():
                a = a.float().contiguous()
            return a, C.c_void_p(a.data_ptr()), (_lib.VP_MEM_DEVICE if a.is_cuda else _lib.VP_MEM_HOST)
        a = np.ascontiguousarray(a, dtype=np.float32)
        return a, _lib.ptr(a), _lib.VP_MEM_HOST

    def _xy(self, x, y):
        """The inputs of a step, checked: ``(x kept, its pointer, y kept, its pointer, mem)``."""
        if tuple(x.shape) != tuple(y.shape) or x.ndim != 3 or x.shape[1] != 3 or x.shape[2] != self.in_samples:
            raise ValueError(f"expected x and y of shape (B, 3, {self.in_samples}), got {tuple(x.shape)} / {tuple(y.shape)}")
        xk, xp, xm = self._arg(x)
        yk, yp, ym = self._arg(y)
        if xm != ym:
            raise ValueError("x and y must both be host arrays or both be device tensors")
        return xk, xp, yk, yp, xm

    def synchronize(self):
        _lib.check(self._c("synchronize")(self._h))

    def _read(self, which):
        out = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self._c("read")(self._h, which, _lib.ptr(out), out.size), self._prefix + "_read")
        return out

    def _named(self, blob):
        shapes = {k: s for k, s, is_param in self.model._state_layout if is_param}
        out, off = {}, 0
        for key, n in self.names:
            out[key] = blob[off:off + n].reshape(shapes[key])
            off += n
        return out

    def weights(self):
        return self._named(self._read(0))

    def gradients(self):
        return self._named(self._read(1))

    def adam_state(self):
        return self._named(self._read(2)), self._named(self._read(3))

    def write_weights(self, blob):
        """Replace the flat blob of ``names`` (for PhaseNet: weights and BatchNorm running statistics, the layout of
        ``model._weights``).  The Adam moments, the update count and the EMA stay as they are (``<_prefix>_write_weights``)."""
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        if blob.shape != (self.n_params,):
            raise ValueError(f"expected a flat blob of {self.n_params} floats, got shape {blob.shape}")
        _lib.check(self._c("write_weights")(self._h, _lib.ptr(blob), blob.size), self._prefix + "_write_weights")


class PhaseNetTrainer(_Trainer):
    """One device-resident PhaseNet with its gradients and Adam state."""

    DTYPES = {"fp32": _lib.VP_TRAIN_FP32, "float32": _lib.VP_TRAIN_FP32, "32": _lib.VP_TRAIN_FP32, "32-true": _lib.VP_TRAIN_FP32,
              "bf16": _lib.VP_TRAIN_BF16, "bfloat16": _lib.VP_TRAIN_BF16, "bf16-mixed": _lib.VP_TRAIN_BF16}
    _prefix, _model_type, _wrong_model = "vp_train", PhaseNet, "the training step is implemented for PhaseNet"

    def __init__(self, model: PhaseNet, max_batch=512, device=0, betas=(0.9, 0.999), eps=1e-8, bn_momentum=0.1,
                 loss_eps=1e-5, dtype="fp32"):
        """``dtype="bf16"``: activation and gradient tensors stored as bfloat16 with fp32 accumulation, fp32 master
        weights, statistics and Adam state (Lightning's ``precision="bf16-mixed"`` in spirit; BASELINE config 5);
        ``"fp32"`` (default) is what the reference's trainer runs."""
        if str(dtype) not in self.DTYPES:
            raise ValueError(f"dtype must be one of {sorted(self.DTYPES)}, got {dtype!r}")
        self.dtype = "bf16" if self.DTYPES[str(dtype)] == _lib.VP_TRAIN_BF16 else "fp32"
        self._check_model(model)
        lib, kind = _lib.load(), _lib.VP_MODEL_PHASENET
        names = [(lib.vp_param_name(kind, i).decode(), int(lib.vp_param_size(kind, i))) for i in range(lib.vp_param_count(kind))]
        self._in_flight = collections.deque()  # (number of a queued step, its x, its y): device inputs kept alive
        super().__init__(model, max_batch, names, (betas[0], betas[1], eps, bn_momentum, loss_eps),
                         lambda lib, w, h: lib.vp_train_create_dtype(int(device), kind, _lib.ptr(w), w.size, int(max_batch),
                                                                     self.DTYPES[str(dtype)], h))

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_in_flight", None):
            self._lib.vp_train_synchronize(self._h)
            self._in_flight.clear()
        super().close()
        self._last_inputs = None

    def step(self, x, y, lr, update=True, want_loss=True, inputs_unchanged=False):
        """Forward + loss + backward (+ Adam when ``update``).  x, y: (B, 3, 3001).

        ``inputs_unchanged=True`` is the caller's PROMISE that x and y are the very tensors of the previous step and that
        nothing has written to them since, by any route (a benchmark re-running one batch): the trainer's stream then does not
        wait for the producer stream again.  It is never inferred: torch's ``Tensor._version`` does not see writes through
        ``x.data``, raw-pointer kernels (this library's own device writers, DLPack consumers) or collective outputs, and a
        loader that refills a persistent buffer that way would be read half-filled."""
        xk, xp, yk, yp, xm = self._xy(x, y)
        self._drop_consumed()
        if xm == _lib.VP_MEM_DEVICE:
            # the trainer runs on its own stream: x / y (or their fp32 copies made above) must be complete first.  An
            # event recorded on torch's stream that the trainer's stream waits for (hipStreamWaitEvent): the host does
            # not block, so a data loader filling the next batch on torch's stream keeps running
            # (The wait is a marker in the trainer's queue in front of the step's first launch, ~25 us of the step; skipped only
            # on the caller's explicit promise -- and then only for the very OBJECTS of the previous step, held here so that
            # their identity cannot be recycled -- or when the producer has already finished.)
            torch = _torch()
            producer = torch.cuda.current_stream(xk.device)
            last = getattr(self, "_last_inputs", None)
            same = bool(inputs_unchanged) and last is not None and last[0] is xk and last[1] is yk and last[2] == producer.cuda_stream
            self._last_inputs = (xk, yk, producer.cuda_stream)
            if not same:
                ev = torch.cuda.Event()
                ev.record(producer)
                if not ev.query():  # (already complete -- a batch prepared well ahead: nothing to wait for either)
                    if getattr(self, "_ext_stream", None) is None:
                        self._ext_stream = torch.cuda.ExternalStream(int(self._lib.vp_train_stream(self._h)), device=xk.device)
                    self._ext_stream.wait_event(ev)
        loss = C.c_double(float("nan"))
        _lib.check(self._lib.vp_train_step(self._h, xp, yp, xm, int(x.shape[0]), float(lr), int(bool(update)),
                                           C.byref(loss) if want_loss else None), "vp_train_step")
        if xm == _lib.VP_MEM_DEVICE:
            # The step is (or may be) still queued on the trainer's non-blocking stream and reads x / y there:
            #  * this object keeps x / y (or the fp32 copies `_arg` made) alive until the library reports the step's last
            #    read of them complete (`_drop_consumed`), so the caching allocator cannot hand their memory out while the step
            #    reads it, whatever the caller does with its own references.  (Not Tensor.record_stream: the allocator would
            #    then record events on the trainer's stream when the tensors die -- possibly after vp_train_destroy has
            #    destroyed that stream.)
            #  * torch's current stream waits -- on the device, the host does not block -- for the event behind the step's
            #    last read of x / y, so `x.copy_(next_batch)` or any other refill enqueued there cannot overtake the step.
            self._in_flight.append((int(self._lib.vp_train_steps_enqueued(self._h)) - 1, xk, yk))
            cur = torch.cuda.current_stream(xk.device)
            _lib.check(self._lib.vp_train_wait_inputs_consumed(self._h, C.c_void_p(cur.cuda_stream)), "vp_train_wait_inputs_consumed")
        self.forward_count = getattr(self, "forward_count", 0) + 1  # every step moves the BatchNorm running statistics
        if update:
            self.global_step += 1
        return loss.value if want_loss else None

    def step_bank(self, bank, rows, lr, sigma, update=True, want_loss=True):
        """``step`` on a batch generated on the GPU: the plan rows (``generate.PLAN_ROW``, e.g. from
        ``WindowPlanner``) are cut from ``bank`` (a ``WaveformBank`` on the trainer's device), normalised with
        ``model.norm`` and labelled with Gaussians of width ``sigma`` in ``model.labels`` order, straight into the
        trainer's input buffers on its own stream (``vp_train_step_bank``).  ``AUG_ROW`` records (``AugmentedPlanner``)
        add the stacking, gap and second normalisation (``vp_train_step_bank_aug``).  ``rows`` may be reused at once."""
        from .generate import AUG_ROW, as_aug_rows, as_rows, label_rows, _norm

        aug = getattr(rows, "dtype", None) == AUG_ROW
        rows = as_aug_rows(rows) if aug else as_rows(rows)
        name = "vp_train_step_bank_aug" if aug else "vp_train_step_bank"
        lrows = label_rows(self.model.labels)
        self._drop_consumed()
        loss = C.c_double(float("nan"))
        _lib.check(getattr(self._lib, name)(self._h, bank.handle, _lib.ptr(rows), len(rows), float(sigma),
                                            _norm(self.model.norm), lrows.ctypes.data_as(C.POINTER(C.c_int)), float(lr),
                                            int(bool(update)), C.byref(loss) if want_loss else None), name)
        # the bank stays referenced until the step's reads of it are complete (as the device inputs of `step`)
        self._in_flight.append((int(self._lib.vp_train_steps_enqueued(self._h)) - 1, bank, None))
        self.forward_count = getattr(self, "forward_count", 0) + 1
        if update:
            self.global_step += 1
        return loss.value if want_loss else None

    def _drop_consumed(self):
        """Device inputs of the steps the trainer's stream has read to the end may go (no event of ours enters that stream:
        the library keeps one per step behind the last reader of x / y and answers which of them have completed)."""
        if self._in_flight:
            upto = int(self._lib.vp_train_inputs_consumed_upto(self._h))
            while self._in_flight and self._in_flight[0][0] <= upto:
                self._in_flight.popleft()

    def synchronize(self):
        super().synchronize()
        self._in_flight.clear()

    def enable_ema(self, decay=0.999):
        """Exponential moving average of the weights after every update (train.py:153-176 of the reference)."""
        _lib.check(self._lib.vp_train_set_ema(self._h, float(decay)), "vp_train_set_ema")

    def ema_weights(self):
        return self._named(self._read(4))

    def predictions(self, B):
        out = np.empty((B, 3, self.in_samples), dtype=np.float32)
        _lib.check(self._lib.vp_train_predictions(self._h, _lib.ptr(out), B))
        return out

    def tensors(self, B):
        """Every z / a / gz / ga tensor of the last step as (B, C, L) arrays, by name (parity tests)."""
        lib, out = self._lib, {}
        for i in range(lib.vp_train_tensor_count(self._h)):
            name, c, l = C.c_char_p(), C.c_int(), C.c_int()
            _lib.check(lib.vp_train_tensor_info(self._h, i, C.byref(name), C.byref(c), C.byref(l)))
            a = np.empty((B, c.value, l.value), dtype=np.float32)
            _lib.check(lib.vp_train_tensor_read(self._h, i, B, _lib.ptr(a)))
            out[name.value.decode()] = a
        return out

    def export(self, ema=False):
        """Copy the trained weights (and BatchNorm running statistics) back into ``self.model``;
        ``ema=True`` exports the EMA weights instead (``enable_ema`` must have been called)."""
        sd = self.model.state_dict()
        sd.update(self.ema_weights() if ema else self.weights())
        for k in sd:
            if k.endswith("num_batches_tracked"):
                sd[k] = np.asarray(sd[k] + self.global_step - getattr(self, "_exported_at", 0))
        self._exported_at = self.global_step
        self.model.load_state_dict(sd)
        return self.model


def _torch():
    import torch

    return torch


class ReduceLROnPlateau:
    """The arithmetic of ``torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min")`` on one learning rate, without torch:
    ``step(metric, lr)`` returns the learning rate that follows ``lr``.  ``is_better`` (relative or absolute threshold
    against the best metric so far), the count of bad epochs, the cooldown in which bad epochs are ignored, the reduction
    ``max(lr * factor, min_lr)`` once the count exceeds ``patience``, and the rule that a reduction of at most ``eps`` is
    skipped (the count and the cooldown restart all the same) are torch's, statement for statement."""

    def __init__(self, factor=0.1, patience=10, min_lr=0.0, threshold=1e-4, threshold_mode="rel", cooldown=0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError(f"threshold mode {threshold_mode} is unknown!")
        self.factor, self.patience, self.min_lr = factor, patience, min_lr
        self.threshold, self.threshold_mode, self.cooldown, self.eps = threshold, threshold_mode, cooldown, eps
        self.best = float("inf")
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def is_better(self, a, best):
        if self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        return a < best - self.threshold

    @property
    def in_cooldown(self):
        return self.cooldown_counter > 0

    def step(self, metric, lr):
        current = float(metric)
        self.last_epoch += 1
        if self.is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.in_cooldown:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0  # bad epochs in the cooldown do not count
        if self.num_bad_epochs > self.patience:
            old_lr = float(lr)
            new_lr = max(old_lr * self.factor, self.min_lr)
            if old_lr - new_lr > self.eps:
                lr = new_lr
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        return lr


LR_SCHEDULERS = {"ReduceLROnPlateau": ReduceLROnPlateau}
VALIDATION_MODES = ("host", "device")


def _fit_scheduler(lr_scheduler, lr_scheduler_args, val_bank, keep_best, early_stop_patience):
    """The checks every ``fit_bank`` makes of what follows the validation loss; returns the scheduler or ``None``."""
    if lr_scheduler is not None and lr_scheduler not in LR_SCHEDULERS:
        raise ValueError(f"lr_scheduler must be None or one of {sorted(LR_SCHEDULERS)}, got {lr_scheduler!r}")
    if val_bank is None and (lr_scheduler is not None or keep_best or early_stop_patience is not None):
        raise ValueError("lr_scheduler, keep_best and early_stop_patience follow the validation loss: they need val_bank")
    return LR_SCHEDULERS[lr_scheduler](**(lr_scheduler_args or {})) if lr_scheduler is not None else None


def _fit_loop(lit, tr, steps, planner, val_planner, scheduler, keep_best, early_stop_patience, step, validation_losses,
              validated_weights):
    """The host side of ``fit_bank`` for either model's lit: epochs of ``planner`` until ``steps`` optimiser steps, the
    warm-up of ``lit.learning_rate``, a validation after every completed epoch and after the last step, and what the
    validation loss drives (scheduler, ``lit.best_state``, early stop; ``lit.history``).  ``step(rows, lr)`` runs one
    optimiser step of ``tr`` and returns its loss, ``validation_losses()`` the batch losses of one validation pass,
    ``validated_weights()`` a host copy of the weights that pass scored."""
    losses, val_losses = [], []
    lit.history = history = {"val_loss": val_losses, "lr": [], "best": None, "stopped_early": False}
    lit.best_state = None
    # the optimiser's learning rate, a state only where a scheduler writes it too
    lr_now = lit.learning_rate(tr.global_step)
    since_best = 0

    def validate():
        nonlocal lr_now, since_best
        val_losses.append(float(np.mean(validation_losses())))
        if scheduler is not None:
            lr_now = scheduler.step(val_losses[-1], lr_now)
        history["lr"].append(lr_now if scheduler is not None else lit.learning_rate(tr.global_step))
        since_best += 1
        if val_losses[-1] < (float("inf") if history["best"] is None else history["best"][2]):  # (never a NaN)
            history["best"] = (len(val_losses) - 1, tr.global_step, val_losses[-1])
            since_best = 0
            if keep_best:
                lit.best_state = validated_weights()
        if early_stop_patience is not None and since_best >= early_stop_patience:
            history["stopped_early"] = True

    while len(losses) < steps and not history["stopped_early"]:
        for rows in planner.epoch():
            k = tr.global_step
            losses.append(step(rows, lit.learning_rate(k) if scheduler is None else lr_now))
            if scheduler is not None and k < lit.WARMUP_STEPS:
                lr_now = lit.lr * (k + 1) / float(lit.WARMUP_STEPS)
            if len(losses) == steps:
                break
        else:
            if val_planner is not None and len(losses) < steps:
                validate()
    if val_planner is None:
        return losses
    if not history["stopped_early"]:
        validate()
    return losses, val_losses


def validate_batches(model, bank, batches, sigma, eps=1e-5, predictions=False):
    """One validation pass on the GPU (``vp_validate_begin`` ... ``vp_validate_end``): every element of ``batches`` (plan
    rows or augmented rows, any number per batch) is cut from ``bank``, run through ``model``'s inference path and scored
    with ``vector_cross_entropy`` in float64 on the device; the host waits once, at the end.  Returns
    ``(batch_losses, window_losses)``: a float64 array with one loss per batch and one with one per window, in order;
    with ``predictions=True`` also the list of the batches' (B, 3, T) predictions (CUDA tensors)."""
    from .generate import label_rows

    lrows = label_rows(model.labels)
    batch, window, _, preds = _validation_pass(model, bank, batches, "vp_validate", lrows, sigma, (float(eps),), False, predictions)
    return (batch, window, preds) if predictions else (batch, window)


def _validation_pass(model, bank, batches, prefix, lrows, sigma, tail, with_heads, predictions):
    """``<prefix>_begin``, ``<prefix>_bank`` or ``<prefix>_bank_aug`` per element of ``batches`` (by the rows' dtype; ``tail``:
    the call's arguments between ``label_rows`` and ``pred_out_dev``), ``<prefix>_end``.  Returns ``(batch_losses,
    window_losses, head_values or None, predictions)``, the head values (n_windows, 3) by row of y."""
    from .evaluate import prediction_tensor
    from .generate import AUG_ROW, as_aug_rows, as_rows, _norm

    lib = _lib.load()
    if model._device_index is None:
        model.cuda(bank.device)
    h = model._ensure_handle()
    preds, n_windows, n_batches = [], 0, 0
    _lib.check(getattr(lib, prefix + "_begin")(h), prefix + "_begin")
    try:
        for rows in batches:
            aug = getattr(rows, "dtype", None) == AUG_ROW
            rows = as_aug_rows(rows) if aug else as_rows(rows)
            name = prefix + ("_bank_aug" if aug else "_bank")
            if predictions:
                preds.append(prediction_tensor(model, len(rows)))
            _lib.check(getattr(lib, name)(h, bank.handle, _lib.ptr(rows), len(rows), float(sigma), _norm(model.norm),
                                          lrows.ctypes.data_as(C.POINTER(C.c_int)), *tail,
                                          C.c_void_p(preds[-1].data_ptr()) if predictions else None), name)
            n_batches += 1
            n_windows += len(rows)
    finally:
        batch = np.empty(n_batches, np.float64)
        window = np.empty(n_windows, np.float64)
        heads = np.empty((n_windows, 3), np.float64) if with_heads else None
        nb, nw = C.c_longlong(), C.c_longlong()
        dp = C.POINTER(C.c_double)
        rc = getattr(lib, prefix + "_end")(h, batch.ctypes.data_as(dp), n_batches, C.byref(nb), window.ctypes.data_as(dp),
                                           *((heads.ctypes.data_as(dp),) if with_heads else ()), n_windows, C.byref(nw))
    _lib.check(rc, prefix + "_end")
    assert (nb.value, nw.value) == (n_batches, n_windows)
    return batch, window, heads, preds


class _Lit:
    """What the two models' lits share: the warm-up of the learning rate, the label check, the trainer made on first use
    (``_ensure``, the subclass's) and the two small rules of the bank loops."""

    WARMUP_STEPS = 500

    def __init__(self, lr, sigma, prob_label_shape, max_batch, device):
        if prob_label_shape != "gaussian":
            raise ValueError(f"prob_label_shape {prob_label_shape!r}: only 'gaussian' labels are implemented (every "
                             "reference config uses them)")
        self.prob_label_shape = prob_label_shape
        self.lr = float(lr)
        self.sigma = sigma
        self._trainer = None
        self._max_batch, self._device = max_batch, device

    def learning_rate(self, step):
        """lr used by optimiser step number ``step`` (0-based).  Step 0 runs at ``lr`` (the optimiser's initial
        value).  The reference's ``optimizer_step`` hook (models.py:177-185, :562-570) runs with ``trainer.global_step`` = the
        steps completed BEFORE the current one (Lightning counts the step after the hook returns), so after step k it
        sets lr * (k + 1) / 500 for step k + 1: step s >= 1 uses lr * s / 500, and the full lr is reached at step 500."""
        if step == 0 or step >= self.WARMUP_STEPS:
            return self.lr
        return self.lr * step / float(self.WARMUP_STEPS)

    @property
    def trainer_state(self):
        return self._ensure()

    @staticmethod
    def _batches(planner_or_rows):
        """The batches of a planner (its ``validation()``), of one array of rows (one batch) or of an iterable of such arrays."""
        if hasattr(planner_or_rows, "validation"):
            return planner_or_rows.validation()
        if getattr(getattr(planner_or_rows, "dtype", None), "names", None):
            return [planner_or_rows]
        return planner_or_rows

    @staticmethod
    def _check_full_batch(bank, batch_size):
        if len(bank.lengths) < batch_size:
            raise ValueError(f"a bank of {len(bank.lengths)} traces holds no full batch of {batch_size}")


class PhaseNetLit(_Lit):
    """The arithmetic of the reference's ``PhaseNetLit`` (models.py:108-185): Adam at ``lr`` with the
    500-step linear warm-up of ``optimizer_step``.  ``training_step(batch)`` takes
    ``{"X": (B, 3, 3001), "y": (B, 3, 3001)}`` and performs forward, loss, backward AND the
    optimiser step (Lightning's loop does the last two around the reference's ``training_step``)."""

    def __init__(self, lr=1e-2, sigma=20, max_batch=512, model=None, device=0, precision="32", prob_label_shape="gaussian",
                 **model_kwargs):
        super().__init__(lr, sigma, prob_label_shape, max_batch, device)
        self.precision = str(precision)  # "32" (the reference's) or "bf16-mixed" (PhaseNetTrainer dtype="bf16")
        self.model = model if model is not None else PhaseNet(**model_kwargs)
        self._ema = False

    def _ensure(self):
        if self._trainer is None:
            self._trainer = PhaseNetTrainer(self.model, max_batch=self._max_batch, device=self._device, dtype=self.precision)
        return self._trainer

    def training_step(self, batch, batch_idx=None):
        tr = self._ensure()
        return tr.step(batch["X"], batch["y"], self.learning_rate(tr.global_step), update=True)

    def _exported_model(self):
        """``self.model`` on the GPU with the trainer's current weights (the EMA weights when EMA is on), exported only
        when something has changed since the last export."""
        tr = self._ensure()
        # what the exported model depends on: the weights (global_step), the BatchNorm running statistics (every
        # step(), update or not, moves them) and which weights are validated (EMA on / off)
        key = (tr.global_step, getattr(tr, "forward_count", 0), self._ema)
        if getattr(self, "_validated_at", None) != key:
            model = tr.export(ema=self._ema)
            self._validated_at = key
        else:
            model = self.model
        if model._device_index is None:
            model.cuda(self._device)
        return model

    def validation_step(self, batch, batch_idx=None):
        """Loss in eval mode (running statistics), as Lightning's validation loop computes it: the current weights
        go through the inference path (``vp_forward``).  The device plan is rebuilt only when an optimiser step
        has happened since the last validation batch.  With EMA enabled (``enable_ema``) the EMA weights are the
        ones validated, as the reference's EMA callback does with ``validate_original_weights=False``
        (volpick/model/ema.py)."""
        model = self._exported_model()
        p = model(batch["X"])
        p = p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
        y = batch["y"]
        y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        return vector_cross_entropy(p.astype(np.float64), y.astype(np.float64))

    def validate_bank(self, val_bank, planner_or_rows, per_window=False):
        """The validation loss of every batch of ``planner_or_rows`` -- a planner (its ``validation()`` batches), one array of
        rows (one batch) or an iterable of such arrays -- on the GPU from end to end: the current weights (the EMA weights when EMA is on) are
        exported as ``validation_step`` exports them, then one ``validate_batches`` pass generates, predicts and scores the
        batches with a single host wait.  Returns the list of batch losses; with ``per_window=True``
        ``(batch_losses, window_losses)``, the latter one float64 array over all windows in order."""
        model = self._exported_model()
        batches = self._batches(planner_or_rows)
        batch, window = validate_batches(model, val_bank, batches, self.sigma)
        return (batch.tolist(), window) if per_window else batch.tolist()

    def fit_bank(self, bank, steps, batch_size=512, seed=0, val_bank=None, augment=None, validation="host",
                 lr_scheduler=None, lr_scheduler_args=None, keep_best=False, early_stop_patience=None):
        """``steps`` optimiser steps on batches generated on the GPU from ``bank`` (a ``WaveformBank``): epochs of
        ``WindowPlanner(bank, batch_size, seed=seed)`` (a new permutation each, last partial batch dropped), learning
        rate ``learning_rate(step)``, labels of width ``self.sigma``.  Returns the per-step losses and, with ``val_bank``,
        ``(losses, val_losses)``: the mean ``validation_step`` loss over ``val_bank`` (in order, the last partial batch
        kept, its own planner seeded ``seed + 1``) after every completed epoch and after the last step.

        ``augment`` (a ``generate.Augmentation``) adds the reference's stacking block, gap and second Normalize to the
        training and the validation batches (``AugmentedPlanner`` with its subsets of ``bank`` / ``val_bank``); ``None``
        plans block 1 alone.

        ``validation="device"`` computes the same validation loss -- the unweighted mean of the batch losses -- with
        ``validate_bank``: batches, predictions and losses stay on the GPU.

        What the validation loss drives (the reference's ``configure_optimizers`` and ``train.py`` callbacks; all need
        ``val_bank``):

        * ``lr_scheduler="ReduceLROnPlateau"`` with ``lr_scheduler_args`` (``factor``, ``patience``, ``min_lr``, ...): stepped
          with the validation loss after every validation (Lightning's ``interval="epoch"``, monitor ``val_loss``).  The
          optimiser then has ONE learning rate that both the warm-up and the scheduler write: after optimiser step
          ``k < WARMUP_STEPS`` the warm-up sets it to ``lr * (k + 1) / WARMUP_STEPS``, overwriting a reduction made
          meanwhile; from step ``WARMUP_STEPS`` on only the scheduler changes it, by ``max(current * factor, min_lr)``.
          The scheduler's state lasts for this call.
        * ``keep_best=True`` keeps in ``self.best_state`` a host copy of the validated weights (``weights()``, the EMA
          weights when EMA is on) of the strictly lowest validation loss so far (``ModelCheckpoint(mode="min")``).
        * ``early_stop_patience=n`` ends the fit after ``n`` validations in a row without a new minimum.

        ``self.history`` records the call: ``val_loss`` per validation, ``lr`` in force after each of them, ``best`` =
        (validation index, global step, loss) of the minimum or ``None``, and ``stopped_early``."""
        from .generate import WindowPlanner

        if validation not in VALIDATION_MODES:
            raise ValueError(f"validation must be one of {VALIDATION_MODES}, got {validation!r}")
        scheduler = _fit_scheduler(lr_scheduler, lr_scheduler_args, val_bank, keep_best, early_stop_patience)
        tr = self._ensure()
        in_samples = self.model.in_samples
        if augment is None:
            planner = WindowPlanner(bank, batch_size, in_samples=in_samples, seed=seed)
        else:
            planner = augment.planner(bank, batch_size, seed, in_samples=in_samples, sigma=self.sigma)
        self._check_full_batch(bank, batch_size)
        val_planner = None
        if val_bank is not None and augment is None:
            val_planner = WindowPlanner(val_bank, batch_size, in_samples=in_samples, seed=seed + 1)
        elif val_bank is not None:
            val_planner = augment.planner(val_bank, batch_size, seed + 1, in_samples=in_samples, sigma=self.sigma,
                                          validation=True)

        def validation_losses():
            if validation == "device":
                return self.validate_bank(val_bank, val_planner)
            return [self.validation_step(val_bank.make_batch(rows, self.model, self.sigma)) for rows in val_planner.validation()]

        return _fit_loop(self, tr, steps, planner, val_planner, scheduler, keep_best, early_stop_patience,
                         step=lambda rows, lr: tr.step_bank(bank, rows, lr, self.sigma), validation_losses=validation_losses,
                         validated_weights=lambda: tr.ema_weights() if self._ema else tr.weights())

    def enable_ema(self, decay=0.999):
        self._ensure().enable_ema(decay)
        self._ema = True


def validate_batches_eqt(model, bank, batches, sigma, loss_weights=EQT_LOSS_WEIGHTS, detection_fixed_window=None,
                         predictions=False):
    """One validation pass of an EQTransformer on the GPU (``vp_validate_eqt_begin`` ... ``vp_validate_eqt_end``): every
    element of ``batches`` (plan rows, or augmented rows of the stacked recipe -- ``vp_validate_eqt_bank_aug``; any number per
    batch, both kinds in one pass) is cut from ``bank`` and labelled as ``make_batch`` / ``make_batch_eqt_aug`` does for the
    model (P, S and the detection box), run through the model's inference path and scored with
    ``loss_weights[0] BCE(detection) + loss_weights[1] BCE(P) + loss_weights[2] BCE(S)`` in float64 on the device; the host
    waits once, at the end.  Returns ``(batch_losses, window_losses, head_losses)``: float64 arrays with one loss per batch,
    one per window and the unweighted (detection, P, S) values per window, (n_windows, 3); with ``predictions=True`` also the
    list of the batches' (B, 3, T) predictions (CUDA tensors)."""
    from .generate import detection_label_rows, _fixed_window

    lrows = detection_label_rows(model.labels)
    w = _loss_weights(loss_weights)
    tail = (_fixed_window(detection_fixed_window), w.ctypes.data_as(C.POINTER(C.c_double)))
    batch, window, heads, preds = _validation_pass(model, bank, batches, "vp_validate_eqt", lrows, sigma, tail, True, predictions)
    heads = heads[:, lrows]  # by row of y -> (detection, P, S)
    return (batch, window, heads, preds) if predictions else (batch, window, heads)


def decoder_param_names():
    """The 48 tensors ``EQTransformerDecoderTrainer`` trains -- ``decoder_d`` with ``conv_d``, ``pick_decoders.{0,1}`` with
    ``pick_convs.{0,1}`` -- as ``[(name, size)]`` in the flat blob's order (``vp_eqt_dec_train_param_name`` / ``_size``)."""
    lib = _lib.load()
    return [(lib.vp_eqt_dec_train_param_name(i).decode(), int(lib.vp_eqt_dec_train_param_size(i)))
            for i in range(lib.vp_eqt_dec_train_param_count())]


def _scope_param_names(scope):
    lib = _lib.load()
    return [(lib.vp_eqt_dec_train_scope_param_name(scope, i).decode(), int(lib.vp_eqt_dec_train_scope_param_size(scope, i)))
            for i in range(lib.vp_eqt_dec_train_scope_param_count(scope))]


def pick_branch_param_names():
    """The 66 tensors of ``EQTransformerDecoderTrainer(scope="pick_branches")`` -- the 48 of ``decoder_param_names`` and
    ``pick_lstms.{0,1}`` with ``pick_attentions.{0,1}`` -- as ``[(name, size)]`` in the flat blob's order: 152,261 floats."""
    return _scope_param_names(TRAIN_SCOPES["pick_branches"])


TRAIN_SCOPES = {"decoders": 0, "pick_branches": 1}  # VP_EQT_TRAIN_DECODERS, VP_EQT_TRAIN_PICK_BRANCHES
EQT_DROP_RATE = 0.1  # SeisBench's EQTransformer default


class EQTransformerDecoderTrainer(_Trainer):
    """The three decoder stacks and heads of one EQTransformer on the device, with their gradients and Adam state; the
    trunk is frozen and runs as the inference path (``vp_eqt_dec_train_*``).  ``PhaseNetTrainer``'s role for
    ``EQTransformerLit(trainable=...)``.  The trainer builds its own device plan from ``model``'s weights and config
    when it is made and does not follow later changes of ``model``; ``export()`` writes the trained tensors back.

    ``scope="decoders"``: the 48 tensors of ``decoder_param_names``.  ``scope="pick_branches"`` adds the pick LSTMs and
    attentions in front of the P and S decoders (``pick_branch_param_names``: 66 tensors) and runs their training forward:
    dropout of rate ``drop_rate`` (``None``: SeisBench's 0.1; 0 switches it off) between each LSTM and its attention, with
    masks that are a function of ``seed``, the count of steps and the element (Philox; ``volpick_amd/csrc/philox.h``).
    ``names``, ``weights()``, ``gradients()``, ``write_weights``, ``export()`` and ``tensors()`` follow the scope."""

    N_SETS = 3  # detection, P, S
    _prefix, _model_type, _wrong_model = "vp_eqt_dec_train", EQTransformer, "the decoder training step is implemented for EQTransformer"

    def __init__(self, model: EQTransformer, max_batch=256, device=0, betas=(0.9, 0.999), eps=1e-8, scope="decoders",
                 drop_rate=None, seed=0):
        self._check_model(model)
        from .generate import detection_label_rows

        if list(detection_label_rows(model.labels)) != [0, 1, 2]:
            raise ValueError(f"the trainer's heads are (Detection, P, S) in this order, the model's labels are {model.labels!r}")
        if scope not in TRAIN_SCOPES:
            raise ValueError(f"scope must be one of {tuple(TRAIN_SCOPES)}, got {scope!r}")
        self.scope = scope
        self.drop_rate = EQT_DROP_RATE if drop_rate is None else float(drop_rate)
        self.seed = int(seed)
        self._held = None  # the device inputs / the bank of the latest step: this trainer's steps return complete
        cfg = model._config()
        super().__init__(model, max_batch, _scope_param_names(TRAIN_SCOPES[scope]), (betas[0], betas[1], eps),
                         lambda lib, w, h: lib.vp_eqt_dec_train_create_scope(int(device), _lib.ptr(w), w.size, C.byref(cfg),
                                                                             int(max_batch), TRAIN_SCOPES[scope], self.drop_rate,
                                                                             self.seed & (2 ** 64 - 1), h))

    def close(self):
        super().close()
        self._held = None

    def step(self, x, y, lr, loss_weights=EQT_LOSS_WEIGHTS, update=True):
        """Forward + loss + backward (+ Adam when ``update``); returns the loss.  x: (B, 3, 6000), normalised; y: (B, 3, 6000)
        with the rows detection, P, S.  Both numpy arrays or both CUDA tensors (complete on torch's current stream: the call
        waits for that stream, and for its own before it returns)."""
        xk, xp, yk, yp, xm = self._xy(x, y)
        if xm == _lib.VP_MEM_DEVICE:
            _torch().cuda.current_stream(xk.device).synchronize()
        self._held = (xk, yk)
        w = _loss_weights(loss_weights)
        loss = C.c_double(float("nan"))
        _lib.check(self._lib.vp_eqt_dec_train_step(self._h, xp, yp, xm, int(x.shape[0]), w.ctypes.data_as(C.POINTER(C.c_double)),
                                                   float(lr), int(bool(update)), C.byref(loss)), "vp_eqt_dec_train_step")
        if update:
            self.global_step += 1
        return loss.value

    def step_bank(self, bank, rows, lr, sigma, loss_weights=EQT_LOSS_WEIGHTS, detection_fixed_window=None, update=True):
        """``step`` on a batch generated on the GPU straight into the trainer's buffers: plan rows as
        ``vp_bank_make_batch_eqt`` executes them, ``AUG_ROW`` records as ``vp_bank_make_batch_eqt_aug`` does (chosen by the
        rows' dtype), normalised with ``model.norm``.  ``rows`` may be reused at once."""
        from .generate import AUG_ROW, as_aug_rows, as_rows, _fixed_window, _norm

        aug = getattr(rows, "dtype", None) == AUG_ROW
        rows = as_aug_rows(rows) if aug else as_rows(rows)
        name = "vp_eqt_dec_train_step_bank_aug" if aug else "vp_eqt_dec_train_step_bank"
        lrows = np.array([0, 1, 2], np.int32)
        w = _loss_weights(loss_weights)
        self._held = bank
        loss = C.c_double(float("nan"))
        _lib.check(getattr(self._lib, name)(self._h, bank.handle, _lib.ptr(rows), len(rows), float(sigma), _norm(self.model.norm),
                                            lrows.ctypes.data_as(C.POINTER(C.c_int)), _fixed_window(detection_fixed_window),
                                            w.ctypes.data_as(C.POINTER(C.c_double)), float(lr), int(bool(update)), C.byref(loss)),
                   name)
        if update:
            self.global_step += 1
        return loss.value

    def write_weights(self, blob):
        """Replace the trained floats (145,731, or 152,261 with the pick branches; the order of ``names``; a dict of the
        tensors is flattened).  The Adam moments and the update count stay as they are (``vp_eqt_dec_train_write_weights``)."""
        if isinstance(blob, dict):
            blob = np.concatenate([np.asarray(blob[k], np.float32).ravel() for k, _ in self.names])
        super().write_weights(blob)

    def tensors(self, B):
        """Every tensor of the last step (a batch of ``B`` windows) by name: ``decoder.in``, ``a0`` .. ``a6``, ``logits``,
        ``gz_head``, ``ga0`` .. ``ga6``, ``gz0`` .. ``gz6`` as (3, B, C, L) arrays -- decoder detection, P, S -- and the
        predictions ``p`` as (B, 3, 6000).  With ``scope="pick_branches"`` also the branches' tensors ``pick.*`` as
        (2, B, C, 47) arrays -- P, S -- and ``pick.x`` (B, 16, 47), listed in include/volpick_hip.h."""
        lib, out = self._lib, {}
        for i in range(lib.vp_eqt_dec_train_tensor_count(self._h)):
            name, s, c, l = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
            _lib.check(lib.vp_eqt_dec_train_tensor_info(self._h, i, C.byref(name), C.byref(s), C.byref(c), C.byref(l)))
            a = np.empty((s.value, B, c.value, l.value), dtype=np.float32)
            _lib.check(lib.vp_eqt_dec_train_tensor_read(self._h, i, B, _lib.ptr(a)))
            out[name.value.decode()] = a[0] if s.value == 1 else a
        return out

    def launch_count(self):
        return int(self._lib.vp_eqt_dec_train_launch_count(self._h))

    def phase_ms(self):
        """(trunk, forward + heads + loss, input gradients, weight gradients, Adam) of the last step in ms; needs
        ``set_timing(True)`` before that step."""
        ms = (C.c_float * 5)()
        _lib.check(self._lib.vp_eqt_dec_train_phase_ms(self._h, ms), "vp_eqt_dec_train_phase_ms")
        return tuple(float(v) for v in ms)

    def pick_ms(self):
        """(forward, adjoints, weight gradients) of the pick branches in the last step in ms, the parts ``phase_ms`` counts
        under its second, third and fourth phase; needs ``scope="pick_branches"`` and ``set_timing(True)`` before that step."""
        ms = (C.c_float * 3)()
        _lib.check(self._lib.vp_eqt_dec_train_pick_ms(self._h, ms), "vp_eqt_dec_train_pick_ms")
        return tuple(float(v) for v in ms)

    def set_timing(self, on=True):
        _lib.check(self._lib.vp_eqt_dec_train_set_timing(self._h, int(bool(on))))

    def export(self):
        """Copy the trained tensors (``names``) back into ``self.model`` (``state_dict`` / ``load_state_dict``); every other tensor
        keeps its bits."""
        sd = self.model.state_dict()
        sd.update(self.weights())
        self.model.load_state_dict(sd)
        return self.model


TRAINABLE = ("decoders", "pick_branches")


class EQTransformerLit(_Lit):
    """The reference's ``EQTransformerLit`` (models.py:483-879): block 1's batch or the stacked recipe's
    (``augmented_planner``; the reference's ``get_val_augmentations`` with ``stack_data``) and ``shared_step``'s loss
    ``loss_weights[0] BCE(detection) + loss_weights[1] BCE(P) + loss_weights[2] BCE(S)``, by which the reference selects its
    checkpoints.  ``validation_step(batch)`` takes what ``WaveformBank.make_batch`` returns for the model:
    ``{"X": (B, 3, 6000), "y": (B, 2, 6000), "detections": (B, 1, 6000)}``.

    ``trainable=None`` (default) validates only: ``training_step`` raises.  ``trainable="decoders"`` trains the three
    decoder stacks and their heads with the trunk frozen (``EQTransformerDecoderTrainer``): ``training_step(batch)`` on the
    same dictionaries and ``fit_bank``.  ``trainable="pick_branches"`` trains the pick LSTMs and attentions in front of the
    P and S decoders as well (``EQTransformerDecoderTrainer(scope="pick_branches", drop_rate=..., seed=...)``: 66 tensors,
    dropout as in training) through the same calls.  Training the rest of the trunk (encoder, ResCNN, BiLSTMs,
    transformers) is not implemented."""

    def __init__(self, lr=1e-2, sigma=20, loss_weights=EQT_LOSS_WEIGHTS, detection_fixed_window=None,
                 prob_label_shape="gaussian", model=None, device=0, trainable=None, max_batch=256, drop_rate=None, seed=0,
                 **model_kwargs):
        super().__init__(lr, sigma, prob_label_shape, max_batch, device)
        self.loss_weights = tuple(float(w) for w in _loss_weights(loss_weights))
        if trainable is not None and trainable not in TRAINABLE:
            raise ValueError("trainable must be None, 'decoders' (the decoder stacks and heads, trunk frozen) or 'pick_branches' "
                             f"(those and the pick LSTMs and attentions), got {trainable!r}")
        self.trainable = trainable
        self.drop_rate, self.seed = drop_rate, seed
        self.detection_fixed_window = detection_fixed_window
        self.model = model if model is not None else EQTransformer(**model_kwargs)

    def _model_on_device(self):
        """``self.model`` on the GPU; with a trainer, holding the trainer's current weights (exported only when an update has
        happened since the last export)."""
        tr = self._trainer
        if tr is not None and getattr(self, "_exported_at", 0) != tr.global_step:
            tr.export()
            self._exported_at = tr.global_step
        if self.model._device_index is None:
            self.model.cuda(self._device)
        return self.model

    def _ensure(self):
        if self.trainable is None:
            raise NotImplementedError("EQTransformer training needs trainable='decoders' (the decoder stacks and heads, trunk "
                                      "frozen) or trainable='pick_branches' (those and the pick LSTMs and attentions); "
                                      "training the rest of the trunk is not implemented: this object validates "
                                      "(validation_step, validate_bank)")
        if self._trainer is None:
            self._trainer = EQTransformerDecoderTrainer(self.model, max_batch=self._max_batch, device=self._device,
                                                        scope=self.trainable, drop_rate=self.drop_rate, seed=self.seed)
        return self._trainer
    def training_step(self, batch, batch_idx=None):
        """``trainable="decoders"`` / ``"pick_branches"``: forward, loss, backward and the Adam step on ``{"X", "y", "detections"}`` (what
        ``make_batch`` returns); returns the loss.  Otherwise raises ``NotImplementedError``."""
        tr = self._ensure()
        det, y = batch["detections"], batch["y"]
        if hasattr(y, "data_ptr"):
            y3 = _torch().cat([det, y], dim=1)
        else:
            y3 = np.concatenate([np.asarray(det), np.asarray(y)], axis=1)
        return tr.step(batch["X"], y3, self.learning_rate(tr.global_step), self.loss_weights, update=True)

    def fit_bank(self, bank, steps, batch_size=256, seed=0, val_bank=None, augment=None, lr_scheduler=None,
                 lr_scheduler_args=None, keep_best=False, early_stop_patience=None):
        """``steps`` optimiser steps of the decoder trainer on batches generated on the GPU from ``bank``: epochs of
        ``window_planner`` (``augment``: of ``augmented_planner``), the warm-up of ``learning_rate``, and -- with ``val_bank`` --
        ``validate_bank`` on the exported weights after every completed epoch and after the last step, which drives
        ``lr_scheduler``, ``keep_best`` (``self.best_state``: the trained tensors -- 48, or 66 with the pick branches -- of the lowest validation loss, restored
        into the trainer and the model when the fit ends) and ``early_stop_patience`` exactly as in ``PhaseNetLit.fit_bank``
        (one shared host loop).  Returns the per-step losses and, with ``val_bank``, ``(losses, val_losses)``."""
        scheduler = _fit_scheduler(lr_scheduler, lr_scheduler_args, val_bank, keep_best, early_stop_patience)
        tr = self._ensure()
        self._check_full_batch(bank, batch_size)
        plan = (lambda b, s, v: self.window_planner(b, batch_size, seed=s)) if augment is None else \
            (lambda b, s, v: self.augmented_planner(b, batch_size, augment, seed=s, validation=v))
        planner = plan(bank, seed, False)
        val_planner = plan(val_bank, seed + 1, True) if val_bank is not None else None
        out = _fit_loop(self, tr, steps, planner, val_planner, scheduler, keep_best, early_stop_patience,
                        step=lambda rows, lr: tr.step_bank(bank, rows, lr, self.sigma, self.loss_weights, self.detection_fixed_window),
                        validation_losses=lambda: self.validate_bank(val_bank, val_planner), validated_weights=tr.weights)
        if keep_best and self.best_state is not None:
            tr.write_weights(self.best_state)
            tr.export()
            self._exported_at = tr.global_step
        return out

    def window_planner(self, bank, batch_size, seed=0):
        """Block 1's windows for this model (models.py:606-652): around a pick with ``samples_before=6000`` in an extent of
        12000 samples, then a random window of 6000."""
        from .generate import WindowPlanner

        return WindowPlanner(bank, batch_size, samples_before=6000, first_windowlen=12000, in_samples=self.model.in_samples,
                             seed=seed)

    def augmented_planner(self, bank, batch_size, augment, seed=0, validation=False):
        """The stacked recipe's windows for this model (models.py:668-844): ``augment`` (a ``generate.Augmentation``) planned
        with block 1's windows above for the primary and the noise sources, ``samples_before=3000`` in an extent of 8000
        samples for the event sources, and this lit's label width."""
        return augment.planner(bank, batch_size, seed, in_samples=self.model.in_samples, sigma=self.sigma, validation=validation,
                               event_samples_before=3000, event_windowlen=8000, samples_before=6000, first_windowlen=12000)

    def make_batch(self, bank, rows):
        """The batch of plan rows (block 1) or of augmented rows (the stacked recipe), by the rows' dtype."""
        from .generate import AUG_ROW

        make = bank.make_batch_eqt_aug if getattr(rows, "dtype", None) == AUG_ROW else bank.make_batch
        return make(rows, self.model, self.sigma, detection_fixed_window=self.detection_fixed_window)

    def validation_step(self, batch, batch_idx=None):
        """``shared_step`` on the host: the model's output copied back, ``bce_loss`` in numpy float64."""
        host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        det, p, s = self._model_on_device()(batch["X"])
        pred = np.stack([host(det), host(p), host(s)], axis=1)
        y = np.concatenate([host(batch["detections"]), host(batch["y"])], axis=1)
        return bce_loss(pred, y, self.loss_weights)

    def validate_bank(self, val_bank, planner_or_rows, per_window=False):
        """The validation loss of every batch of ``planner_or_rows`` -- a planner (its ``validation()`` batches; with an
        ``augmented_planner`` this is the reference's validation pass), one array of rows (one batch) or an iterable of such
        arrays, plan rows or augmented rows -- on the GPU from end to end (``validate_batches_eqt``: one host wait).  Returns the list of batch losses; with ``per_window=True`` ``(batch_losses, window_losses)``, the latter one
        float64 array over all windows in order."""
        batches = self._batches(planner_or_rows)
        batch, window, _ = validate_batches_eqt(self._model_on_device(), val_bank, batches, self.sigma, self.loss_weights,
                                                self.detection_fixed_window)
        return (batch.tolist(), window) if per_window else batch.tolist()
