"""Float64 restatements and a-priori bars of what surrounds the conv / BatchNorm / weight-gradient launches of the PhaseNet
training step (volpick_amd/csrc/train_phasenet.hip, train_kernels.h, train_optim.hip): ``adam_kernel``, the BatchNorm running statistics and
the loss head (``head_fwd_bwd_kernel``, ``head_fwd_bwd_pair_kernel<bf16_t, 4>``, ``head_final_kernel``).  Numpy only; shared
by tests/test_train_state_cpu.py (emulations and mutations) and tests/test_gpu_train_state.py.  Every restatement is fed the
values the update really read (the trainer hands back gradients, moments, weights and stored tensors), so nothing here
inherits the drift of the conv layers and the bars are rounding bars.  None of them is taken from a run of the kernels, with
the one exception named under "Measured" below.

u = 2^-24 (float32 unit roundoff).  An operation's result is off by at most u |result|; a sum of same-signed terms that goes
through D roundings by D u |sum|; where terms cancel, the magnitude is the sum of the absolute terms.  A contraction of
a * b + c into an fma only removes a rounding, so the bars hold for both forms.  FLOOR = 2^-126 per rounding is what a result
below the smallest normal float32 may lose, whether the device keeps denormals or flushes them.

Adam (adam_kernel; b1, b2, eps, lr are the float32 values the C ABI receives, t = updates including this one)
  m' = b1 m + (1 - b1) g             fl(b1 m): u |b1 m|; fl(1 - b1) fl(* g): 2 u |(1 - b1) g| (1 - b1 is exact for b1 >= 1/2);
                                     the sum: u (|b1 m| + |(1 - b1) g|).          bar_m = 3 u (|b1 m| + |(1 - b1) g|)
  v' = b2 v + (1 - b2) g^2           as m' with one more product.                bar_v = 4 u (|b2 v| + (1 - b2) g^2)
  w' = w - step, step = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), bc = 1 - b^t
     The final subtraction: u |w'|.  Relative to |step|: m' 3 u, v' 4 u halved by the root = 2 u, sqrtf u, sqrtf(bc2) u, the
     division by it u, + eps u, m' / denom u, lr / bc1 u, the product u: 12 u if every rounding is at its worst and pulls the
     same way, 10.5 u for betas >= 1/2.  The project's figure is 10 u and is kept: to pass it, nine independent roundings
     would all have to sit within a few per cent of their worst, on the same side.
     The bias corrections are formed in float on the host: powf to one ulp (2 u b^t) and the subtraction (u bc),
     dbc = (2 u b^t + u bc) / bc, bc1 enters the step directly and bc2 under a root.  For beta2 = 0.999, dbc2 is 6e-5 at
     t = 2 (its half, 500 u, is the dominant term) and falls from there.
                                     bar_w(plain) = u |w'| + |step| (10 u + dbc1 + dbc2 / 2)
     Two terms that the plain bar leaves out and that are not roundings of the w' statement:
       * m' cancels when the new gradient opposes the carried moment.  The 3 u above assumes |m'| = |b1 m| + |(1 - b1) g|; what
         bar_m allows beyond 3 u |m'| reaches w' through d step / d m' = (lr / bc1) / denom.  The term is zero for an element
         that does not cancel, so there the bar IS the plain one.  tests/test_train_state_cpu.py shows an unmutated float32
         emulation missing the plain bar on such an element.
       * v' below FLOOR: sqrt(v' + d) - sqrt(v') <= sqrt(d), 2^-62 against a denominator that is at least eps.
  The same bars: an update count off by one misses by 10^3 bars and more, eps inside the root by 10^4 (asserted on the CPU).

Running statistics (bn_finish_stats): float64 mean and UNBIASED variance over (B, L) of the stored z, blended as torch does,
  (1 - momentum) old + momentum new.  Bar: the project's 1e-5 (max|want| + 1e-3) per tensor (check_adam_and_running_statistics).

Head (per sample: logits z = W a + b, e = exp(z - max z), p = e / sum e, q = p + eps, loss term -y log q, g = -y / q * scale,
dot = sum g p, gl = p (g - dot), ga = W^T gl; scale = 1 / (B T); 28 sums over the samples: loss, d bias = sum gl, d weight =
sum gl a).  Float64 throughout.  The bars follow the kernels' operations, S_c = |b_c| + sum_k |w_ck a_k|:
  z_c      8 fmas, each rounding a partial sum <= S_c: 8 u S_c.  The shift is the same number on both sides of the softmax
           (softmax is shift invariant), so only z_c - mx adds: u |z_c - mx|.
  e_c      relative a_c = 8 u S_c + u |z_c - mx| + K_EXP u.
  p_c      the sum of e: 2 u, 1 / sum: K_DIV u, e * inv: u; the normalisation carries sum_j p_j a_j:
           rho_c = a_c + sum_j p_j a_j + (3 + K_DIV) u,   bar_p = p rho + FLOOR (expf underflows to exactly 0 below -103.98).
  q, log   dq = bar_p + u q; the loss term moves by y dq / q, and by K_LOG u |y log q| for logf.
  loss     per sample sum_c y dq / q + (K_LOG + 5) u sum_c |y log q| (the product, two additions, scale and its own
           division); the wave butterfly is 6 additions and the bf16 kernel adds its four samples first, 3 more:
           bar_loss = scale sum_samples [sum_c y dq / q + (K_LOG + 14) u sum_c |y log q|]; float64 from there on.
  g_c      d g = |g| (dq / q + (K_DIV + 2) u) + 2 FLOOR (a Gaussian label's far tail is a denormal float32, and g with it).
           dot: three same-signed fmas, d dot = sum_c (|g| bar_p + p d g) + 3 u |dot| + 3 FLOOR.
  gl_c     g - dot cancels, the magnitude is |g| + |dot|:
           d gl = bar_p (|g| + |dot|) + p (d g + d dot + u (|g| + |dot|)) + u p (|g| + |dot|) + FLOOR.
  ga_k     sum_c |w_ck| d gl_c + 3 u sum_c |w_ck gl_c| + 5 FLOOR; a bf16 row is rounded once more, half a bf16 ulp: 2^-8 |ga|.
  sums     d bias_c: sum d gl + 9 u sum |gl| + u |result|;  d weight_ck: sum |a_k| d gl + 10 u sum |gl a_k| + u |result|
           (product or fma, 3 for the bf16 quad, 6 for the butterfly, the final cast).
  K_DIV = 1: the library is built with hipcc's defaults, under which float division and sqrtf are correctly rounded.

Measured, not derived: K_EXP and K_LOG.  The ulp table of the device's expf and logf is not among the ROCm files of the
build machines, so each is four times a figure measured on an MI355X against this float64 reference (the margin because a
different ``a`` lands on different arguments), recorded in profiles/train_state_gpu_tests.txt: the worst |got - ref| in units
of u times the magnitude the term multiplies (p for expf, over the predictions above 0.01; the bar's sum |y log q| scale for
logf, over the loss), with the shipped weights, over the five steps, three hyper-parameter sets and two dtypes of
tests/test_gpu_train_state.py, and with ALL of the observed error charged to the function -- an upper estimate of its own
share (the figures do not depend on K_EXP / K_LOG; with both at zero every bar was still met).  Figures: expf 13.2, logf 1.63;
K_EXP = 53, K_LOG = 6.5.
"""
import collections

import numpy as np

U = 2.0 ** -24
U_BF16 = 2.0 ** -8  # bfloat16 keeps 8 significant bits: half an ulp is at most 2^-8 of the value
FLOOR = 2.0 ** -126
K_DIV = 1.0
K_EXP = 53.0  # measured: 4 x 13.2, see the docstring
K_LOG = 6.5   # measured: 4 x 1.63, see the docstring

DEFAULT_HYPER = (0.9, 0.999, 1e-8, 0.1, 1e-5)  # beta1, beta2, eps, bn_momentum, loss_eps
HYPER_SETS = (DEFAULT_HYPER, (0.5, 0.9, 1e-3, 0.3, 1e-3), (0.8, 0.99, 1e-6, 1.0, 1e-7))

# BatchNorm module -> the layer whose stored z it normalises
BN_LAYERS = {"in_bn": "inc"}
for _i in range(5):
    BN_LAYERS[f"down_branch.{_i}.1"] = f"down{_i}.same"
    if _i < 4:
        BN_LAYERS[f"down_branch.{_i}.3"] = f"down{_i}.down"
for _j in range(4):
    BN_LAYERS[f"up_branch.{_j}.1"] = f"up{_j}.convT"
    BN_LAYERS[f"up_branch.{_j}.3"] = f"up{_j}.same"


def f32(x):
    """The float32 value the C ABI receives, as a Python float."""
    return float(np.float32(x))


def _dbc(b, t):
    bt = b ** t
    bc = 1.0 - bt
    return bc, (2.0 * U * bt + U * bc) / bc


AdamRef = collections.namedtuple("AdamRef", "m v w bar_m bar_v bar_w bar_w_plain")


def adam_update(w, g, m, v, t, lr, b1, b2, eps):
    """One Adam update in float64 from float32 arrays; see the module docstring for the bars."""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    A, Bt = b1 * m, (1.0 - b1) * g
    C, D = b2 * v, (1.0 - b2) * g * g
    m1, v1 = A + Bt, C + D
    (bc1, dbc1), (bc2, dbc2) = _dbc(b1, t), _dbc(b2, t)
    sbc2 = np.sqrt(bc2)
    denom = np.sqrt(v1) / sbc2 + eps
    step = (lr / bc1) * m1 / denom
    w1 = w - step
    bar_m = 3.0 * U * (np.abs(A) + np.abs(Bt)) + 3.0 * FLOOR
    bar_v = 4.0 * U * (np.abs(C) + D) + 4.0 * FLOOR
    plain = U * np.abs(w1) + np.abs(step) * (10.0 * U + dbc1 + dbc2 / 2.0)
    cancel = (lr / bc1) / denom * (bar_m - 3.0 * U * np.abs(m1))
    under = np.abs(step) * np.sqrt(4.0 * FLOOR) / (sbc2 * denom)
    return AdamRef(m1, v1, w1, bar_m, bar_v, plain + cancel + under, plain)


def running_stats(z, rm, rv, momentum):
    """(running_mean', running_var', bar_mean, bar_var) from the stored z (B, C, L) and the previous values."""
    mom = f32(momentum)
    z = np.asarray(z, np.float64)
    mean, var = z.mean((0, 2)), z.var((0, 2), ddof=1)
    rm1 = (1.0 - mom) * np.asarray(rm, np.float64) + mom * mean
    rv1 = (1.0 - mom) * np.asarray(rv, np.float64) + mom * var
    return rm1, rv1, 1e-5 * (np.abs(rm1).max() + 1e-3), 1e-5 * (np.abs(rv1).max() + 1e-3)


HeadRef = collections.namedtuple(
    "HeadRef", "z p loss ga gb gw bar_p bar_loss bar_ga bar_gb bar_gw eps_share log_mag window_loss")


def head(a, w, b, y, eps, bf16=False, k_exp=None, k_log=None):
    """The loss head in float64.  a (B, 8, T) = the stored up3.same.a, w (3, 8), b (3,), y (B, 3, T), eps = loss_eps.
    Returns values and bars (module docstring); ``eps_share``: the share of the loss whose terms have p < eps;
    ``log_mag``: scale sum |y log q|, the magnitude K_LOG multiplies; ``window_loss``: each window's share of the loss.
    ``bf16``: the kernel of the bf16 rows (four samples per thread, ga rounded to bfloat16)."""
    k_exp = K_EXP if k_exp is None else k_exp
    k_log = K_LOG if k_log is None else k_log
    eps = f32(eps)
    a, w, b, y = (np.asarray(v, np.float64) for v in (a, w, b, y))
    B, _, T = a.shape
    scale = 1.0 / (B * T)
    z = np.einsum("ck,bkt->bct", w, a) + b[None, :, None]
    S = np.einsum("ck,bkt->bct", np.abs(w), np.abs(a)) + np.abs(b)[None, :, None]
    d = z - z.max(1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(1, keepdims=True)
    q = p + eps
    logq = np.log(q)
    terms = y * logq
    window_loss = -terms.sum((1, 2)) * scale
    loss = float(window_loss.sum())
    g = -y / q * scale
    dot = (g * p).sum(1, keepdims=True)
    gl = p * (g - dot)
    ga = np.einsum("ck,bct->bkt", w, gl)
    gb = gl.sum((0, 2))
    gw = np.einsum("bct,bkt->ck", gl, a)
    # bars
    arg = 8.0 * U * S + U * np.abs(d) + k_exp * U
    rho = arg + (p * arg).sum(1, keepdims=True) + (3.0 + K_DIV) * U
    bar_p = p * rho + FLOOR
    dq = bar_p + U * q
    log_mag = float(np.abs(terms).sum() * scale)
    bar_loss = float((np.abs(y) * dq / q).sum() * scale + (k_log + 14.0) * U * log_mag)
    dg = np.abs(g) * (dq / q + (K_DIV + 2.0) * U) + 2.0 * FLOOR
    ddot = (np.abs(g) * bar_p + p * dg).sum(1, keepdims=True) + 3.0 * U * np.abs(dot) + 3.0 * FLOOR
    mag = np.abs(g) + np.abs(dot)
    dgl = bar_p * mag + p * (dg + ddot + U * mag) + U * p * mag + FLOOR
    bar_ga = (np.einsum("ck,bct->bkt", np.abs(w), dgl) + 3.0 * U * np.einsum("ck,bct->bkt", np.abs(w), np.abs(gl))
              + 5.0 * FLOOR)
    if bf16:
        bar_ga = bar_ga + U_BF16 * np.abs(ga) + 2.0 ** -134  # (+ half the smallest bfloat16 denormal)
    bar_gb = dgl.sum((0, 2)) + 9.0 * U * np.abs(gl).sum((0, 2)) + U * np.abs(gb)
    bar_gw = (np.einsum("bct,bkt->ck", dgl, np.abs(a)) + 10.0 * U * np.einsum("bct,bkt->ck", np.abs(gl), np.abs(a))
              + U * np.abs(gw))
    small = p < eps
    eps_share = float(-(terms * small).sum() * scale / loss) if loss != 0.0 else 0.0
    return HeadRef(z, p, loss, ga, gb, gw, bar_p, bar_loss, bar_ga, bar_gb, bar_gw, eps_share, log_mag, window_loss)


def ema_update(ema, w1, decay):
    """d ema + (1 - d) w' in float64 and its bar 2 u (|d ema| + |(1 - d) w'|): one rounding per product and one for the
    sum, whose magnitude is at most the two terms'.  1 - d is exact for d >= 1/2, which covers every decay in use (the
    tests take 0.9; decay 0 is held to bit equality instead)."""
    d = f32(decay)
    A, Bt = d * np.asarray(ema, np.float64), (1.0 - d) * np.asarray(w1, np.float64)
    return A + Bt, 2.0 * U * (np.abs(A) + np.abs(Bt)) + 2.0 * FLOOR


# ------------------------------------------------------------------------------------------------ float32 emulations
F = np.float32


def adam_emulated(w, g, m, v, t, lr, b1, b2, eps, mutation=None):
    """adam_kernel and the host lines in front of it, operation by operation in float32 (numpy rounds every operation;
    no fma).  ``mutation``: one of the wrong forms tests/test_train_state_cpu.py lists."""
    w, g, m, v = (np.asarray(a, F) for a in (w, g, m, v))
    lr, b1, b2, eps = F(lr), F(b1), F(b2), F(eps)
    if mutation == "default_betas":
        b1, b2 = F(0.9), F(0.999)
    if mutation == "default_eps":
        eps = F(1e-8)
    if mutation == "count_off_by_one":
        t = t + 1
    one = F(1.0)
    bc1 = one - F(np.power(b1, F(t)))
    bc2 = one - F(np.power(b2, F(t)))
    bc2_sqrt = bc2 if mutation == "bc2_without_root" else np.sqrt(bc2)
    mi = b1 * m + (one - b1) * g
    vi = b2 * v + (one - b2) * g * g
    if mutation == "eps_inside_root":
        denom = np.sqrt(vi + eps) / bc2_sqrt
    else:
        denom = np.sqrt(vi) / bc2_sqrt + eps
    wi = w - (lr / bc1) * (mi / denom)
    return mi.astype(F), vi.astype(F), wi.astype(F)


def _round_f32(x):
    return np.asarray(x, np.float64).astype(F)


def head_emulated(a, w, b, y, eps, bf16=False, mutation=None):
    """The head kernels' per-sample chain in float32, the wave butterfly in float32, float64 from the wave sums on.  exp and
    log are taken in float64 and rounded once (correctly rounded float32 functions).  Returns (p, ga, loss, gb, gw)."""
    a, w, b, y = (np.asarray(v, F) for v in (a, w, b, y))
    eps = F(1e-5) if mutation == "default_loss_eps" else F(eps)
    B, _, T = a.shape
    one = F(1.0)
    scale = one / (F(B) * (one if mutation == "scale_one_over_B" else F(T)))
    z = np.empty((B, 3, T), F)
    for c in range(3):
        acc = np.full((B, T), b[c], F)
        for k in range(8):
            acc = (w[c, k].astype(np.float64) * a[:, k].astype(np.float64) + acc.astype(np.float64)).astype(F)  # fmaf
        z[:, c] = acc
    mx = np.zeros((B, 1, T), F) if mutation == "unshifted_softmax" else z.max(1, keepdims=True)
    with np.errstate(all="ignore"):
        e = _round_f32(np.exp((z - mx).astype(np.float64)))
        inv = one / ((e[:, 0] + e[:, 1]) + e[:, 2])
        p = e * inv[:, None]
        if mutation == "eps_outside_log":
            logq = _round_f32(np.log(p.astype(np.float64))) + eps
        else:
            logq = _round_f32(np.log((p + eps).astype(np.float64)))
        loss = np.zeros((B, T), F)
        dot = np.zeros((B, T), F)
        g = np.empty_like(p)
        for c in range(3):
            loss = loss - y[:, c] * logq[:, c]
            g[:, c] = -y[:, c] / (p[:, c] + eps) * scale
            dot = (g[:, c].astype(np.float64) * p[:, c].astype(np.float64) + dot.astype(np.float64)).astype(F)
        gl = p * (g - dot[:, None])
    ga = np.stack([w[0, k] * gl[:, 0] + w[1, k] * gl[:, 1] + w[2, k] * gl[:, 2] for k in range(8)], 1)
    vals = np.empty((28, B, T), F)
    vals[0] = loss * scale
    for c in range(3):
        vals[1 + c] = gl[:, c]
        for k in range(8):
            vals[4 + 8 * c + k] = gl[:, c] * a[:, k]
    ns = 4 if bf16 else 1
    span = 256 * ns
    nblk = -(-T // span)
    pad = np.zeros((28, B, nblk * span), F)
    pad[:, :, :T] = vals
    lanes = pad.reshape(28, B, nblk, 256, ns)
    per_thread = lanes[..., 0].copy()
    for u in range(1, ns):
        per_thread = per_thread + lanes[..., u]
    waves = per_thread.reshape(28, B, nblk, 4, 64)
    o = 32
    while o:  # the xor butterfly leaves lane 0 the pairwise tree
        waves = waves[..., :o] + waves[..., o:2 * o]
        o //= 2
    sums = waves[..., 0].astype(np.float64).sum((1, 2, 3))
    if bf16:
        ga = round_bf16(ga)
    return p, ga, float(sums[0]), sums[1:4].astype(F), sums[4:].astype(F).reshape(3, 8)


def round_bf16(x):
    """float32 -> bfloat16 (round to nearest even) -> float32."""
    bits = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(F).reshape(np.shape(x))


def running_emulated(z, rm, rv, momentum, mutation=None):
    """bn_finish_stats: float64 sums, biased variance -> unbiased, the blend in float32."""
    mom = F(0.1) if mutation == "default_momentum" else F(momentum)
    z = np.asarray(z, np.float64)
    N = z.shape[0] * z.shape[2]
    mean = z.sum((0, 2)) / N
    var = np.maximum((z * z).sum((0, 2)) / N - mean * mean, 0.0)
    if mutation != "biased_variance":
        var = var * N / (N - 1.0)
    one = F(1.0)
    return ((one - mom) * np.asarray(rm, F) + mom * mean.astype(F)).astype(F), \
           ((one - mom) * np.asarray(rv, F) + mom * var.astype(F)).astype(F)


def ratio(got, want, bar):
    """Worst |got - want| / bar over the elements: inf for a non-finite got and for any difference where the bar is 0."""
    got, want, bar = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bar, np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(np.max(r))
