"""Helpers of the validation-loss tests (not a test module): the float64 oracle of ``vector_cross_entropy`` per window,
its a-priori error bars, the adversarial inputs, and a restatement of the warm-up / ReduceLROnPlateau interaction that
drives a real ``torch.optim.Adam`` parameter group with the real torch scheduler."""
import numpy as np

U = 2.0 ** -53  # unit roundoff of float64


def per_window_loss(p, y, eps=1e-5):
    """L_b = -(1/T) sum_c sum_t y log(p + eps) of (B, C, T) arrays, in numpy float64: mean over samples, sum over classes
    (the reference's order, volpick/model/models.py:43-47)."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        return -(y * np.log(p + eps)).mean(-1).sum(-1)


def bar(p, y, eps=1e-5):
    """Per window: 2 (C T) 2^-53 sum|y log(p + eps)| / T -- the a-priori bound between two summation orders of C T float64
    terms (each order errs by at most (n - 1) u sum|terms| to first order).  A log correct to an ulp or two moves each term
    by a few u |term| and stays far inside it."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    C, T = p.shape[1:]
    with np.errstate(all="ignore"):
        return 2.0 * (C * T) * U * np.abs(y * np.log(p + eps)).sum((-1, -2)) / T


def batch_bar(p, y, eps=1e-5):
    """The bar of the batch loss: the mean of the window bars plus 2 B 2^-53 mean|L_b| for the sum over the windows."""
    L = per_window_loss(p, y, eps)
    return float(bar(p, y, eps).mean() + 2.0 * len(L) * U * np.abs(L).mean())


def kernel_order_loss(p, y, eps=1e-5, nth=256, misalign=None):
    """The window losses summed in the kernel's order (csrc/valloss.hip), emulated in numpy float64: window b of a dense
    array that starts 16-byte aligned has ``(-b n) % 4`` scalar head terms (``misalign``: that count for every window
    instead); thread j adds head term j, the float4 groups j, j + nth, ..., tail term j; a wave's 64 partials fold by
    halves (32, 16, ..., 1), the waves' sums by a tree."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    B, n = p.shape[0], p.shape[1] * p.shape[2]
    out = np.zeros(B)
    with np.errstate(all="ignore"):
        terms = (y * np.log(p + eps)).reshape(B, n)
    for b in range(B):
        t = terms[b]
        head = min(n, (-b * n) % 4 if misalign is None else misalign)
        nvec = (n - head) // 4
        tail = head + 4 * nvec
        part = np.zeros(nth)
        part[:head] += t[:head]
        body = t[head:tail].reshape(nvec, 4)
        for v0 in range(0, nvec, nth):
            chunk = body[v0:v0 + nth]
            for k in range(4):
                part[:len(chunk)] += chunk[:, k]
        part[:n - tail] += t[tail:]
        waves = part.reshape(nth // 64, 64).copy()
        o = 32
        while o:
            waves[:, :o] += waves[:, o:2 * o]
            o //= 2
        red = waves[:, 0].copy()
        s = len(red) // 2
        while s:
            red[:s] += red[s:2 * s]
            s //= 2
        out[b] = -red[0] / p.shape[2]
    return out


def gaussian_y(B, C, T, rng):
    """Labels as the labeller writes them: a Gaussian of width 20 in rows 0 and 1 (where there is one), the rest in the last."""
    t = np.arange(T, dtype=np.float64)
    y = np.zeros((B, C, T))
    for c in range(min(2, C - 1)):
        o = rng.uniform(0, T, B)
        y[:, c] = np.exp(-((t[None] - o[:, None]) ** 2) / (2.0 * 20.0 ** 2))
    y[:, -1] = np.clip(1.0 - y[:, :-1].sum(1), 0.0, 1.0)
    return y.astype(np.float32)


def softmax_p(B, C, T, rng):
    z = rng.normal(0.0, 3.0, (B, C, T))
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def make_inputs(kind, shape, seed=0):
    """(p, y) fp32 of ``shape`` = (B, C, T) for the input kinds of the kernel tests."""
    B, C, T = shape
    rng = np.random.default_rng(seed)
    p, y = softmax_p(B, C, T, rng), gaussian_y(B, C, T, rng)
    if kind == "softmax":
        pass
    elif kind == "p_zero_stretch":  # terms y log(eps): a float eps moves each by 2.5e-8 |y|
        lo = T // 5
        p[:, :, lo:lo + max(1, T // 2)] = 0.0
        y[:, :, lo:lo + max(1, T // 2)] = np.maximum(y[:, :, lo:lo + max(1, T // 2)], 0.25)
    elif kind == "p_one":
        p[:] = 1.0
    elif kind == "y_zero":
        y[:] = 0.0
    elif kind == "p_denormal":
        p[:] = (rng.integers(1, 1 << 22, (B, C, T)) * np.float64(2.0 ** -149)).astype(np.float32)
        assert (p > 0).all() and (p < np.finfo(np.float32).tiny).all()
    else:
        raise ValueError(kind)
    return p, y


INPUT_KINDS = ("softmax", "p_zero_stretch", "p_one", "y_zero", "p_denormal")


def loss_sequences(n, epochs, seed):
    """n seeded validation-loss sequences without NaN: plateaus, slow declines, noise, exact ties."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:  # plateaus with a drop now and then
            level = 1.0 - 0.1 * np.cumsum(rng.random(epochs) < 0.1)
            seq = level + 1e-6 * rng.normal(size=epochs)
        elif kind == 1:  # slow decline around the relative threshold 1e-4 per epoch
            seq = np.cumprod(1.0 - rng.uniform(0.0, 2.5e-4, epochs))
        elif kind == 2:  # noise
            seq = 1.0 + 0.3 * rng.normal(size=epochs)
        else:  # ties: a few values repeated exactly
            seq = rng.choice(np.array([0.5, 0.75, 0.75 * (1 - 1e-4), 1.0]), epochs)
        out.append([float(v) for v in seq])
    return out


def torch_plateau_lrs(losses, lr, **sched_args):
    """The lr after each ``scheduler.step(loss)`` of the real torch ReduceLROnPlateau(mode="min") on an Adam group."""
    import torch

    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", **sched_args)
    out = []
    for v in losses:
        sched.step(v)
        out.append(opt.param_groups[0]["lr"])
    return out


def torch_warmup_plateau(lr, warmup_steps, steps, steps_per_epoch, val_losses, final_validation=True, **sched_args):
    """The learning rates of a fit with the warm-up hook and ReduceLROnPlateau on ONE state, a real Adam group's "lr":

    * optimiser step k (0-based) runs at the group's lr; after it, while k < warmup_steps, the warm-up hook sets
      lr * (k + 1) / warmup_steps (PhaseNetLit.learning_rate's arithmetic), whatever the scheduler had set;
    * after every completed epoch of ``steps_per_epoch`` steps that is not the end of the fit, and (``final_validation``)
      after the last step, the real torch scheduler is stepped with the next of ``val_losses`` (Lightning's
      interval="epoch", monitor "val_loss").

    Returns (lr used by each step, lr after each validation).  Stops early when ``val_losses`` runs out."""
    import torch

    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", **sched_args)
    group = opt.param_groups[0]
    feed = iter(val_losses)
    used, after = [], []

    def validate():
        v = next(feed, None)
        if v is None:
            return False
        sched.step(v)
        after.append(group["lr"])
        return True

    k = 0
    while k < steps:
        for _ in range(steps_per_epoch):
            used.append(group["lr"])
            if k < warmup_steps:
                group["lr"] = lr * (k + 1) / float(warmup_steps)
            k += 1
            if k == steps:
                break
        else:
            if k < steps and not validate():
                return used, after
    if final_validation:
        validate()
    return used, after
