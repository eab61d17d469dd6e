"""Float64 restatements of the two stages around the forward pass, each with an error bound derived from the fp32 arithmetic of
its kernel (volpick_amd/csrc/prepost.hip), the inputs and the case table the CPU and GPU tests share.  Numpy only.

Preprocessing (``gather_normalize_kernel`` and its in-kernel twins): ``pre64``.  Stacking (``stack_kernel``,
``stack_multi_kernel``): ``stack64``.  ``U`` = 2^-24 is the unit roundoff of fp32: one correctly rounded operation has a relative
error of at most U.  A chain of n roundings is bounded by ``gam(n)`` = n U / (1 - n U).  No constant below was taken from a run of
the code under test: each is a count of roundings, with the place in the kernel where they happen."""
import numpy as np

from oracle import constants as OC
from volpick_amd.synthetic import synthetic_windows

U = 2.0 ** -24

# Mean of a channel: s += v[c][k] over MAXE = 6 samples of a thread (the first add is to zero and exact: 5 roundings), the six
# DPP steps of wave_sum3 (6), the 16 wave sums added serially by one thread (acc = 0 + red[0] is exact: 15), the division by T (1).
# Every partial sum is at most sum |x|, so |mean_fp32 - mean| <= gam(C_MU) * mean |x|.
C_MU = 5 + 6 + 15 + 1
# Standard deviation.  Relative roundings on the sum of squares S: d = v - mean (1, which counts twice in d * d), the square (1:
# the kernels write fmaf(d, d, m), which does not round it; counted for a form that does), the thread's serial chain (5), wave_sum (6), the wave sums (acc = r[0]: 15),
# stat[0] + stat[1] + stat[2] of the global form (2): 31; the division by T - 1 or 3T - 1 (1): 32.  The square root halves a
# relative error (16) and rounds once itself (1).
C_SS = (2 + 1 + 5 + 6 + 15 + 2 + 1) // 2 + 1
# The squares are also rounded ABSOLUTELY where they underflow: by at most 2^-126 each if the target flushes fp32 denormals
# (2^-150 if not), so S / (n - 1) by about as much, and sqrt(a + e) - sqrt(a) <= sqrt(e).
STD_UNDERFLOW = 2.0 ** -63
# Output, relative to |o|: den = amp + eps (1); norm_div: v_rcp_f32 and one Newton step leave the reciprocal within one ulp (2),
# q = n * r (1) -- the two residual corrections only improve on that, and they are not relied on, since their residuals may be
# denormal on a tiny window; the taper factor's 1 + cos (1) and the product o * factor (1).  The last two do not happen on the
# untapered samples; the constant is kept uniform.
C_OUT = 1 + 2 + 1 + 1 + 1
# Taper factor 0.5 (1 + cosf(ang)), ABSOLUTE (it is zero at the window's ends): ang = pi_f * (1 + e / 5) with e / 5 (<= 1: U) and
# 1 + .. (<= 2: U) rounded, times pi (2 pi U); pi_f is off by 0.47 U relative (at most 0.94 pi U on ang <= 2 pi); the product
# rounds (2 pi U): 4.94 pi U < 15.6 U on the angle, and |cos'| <= 1.  cosf itself: 2 ulp at |cos| <= 1 (4 U).  Halved by the 0.5.
C_TAP = 10

CONFIGS = [  # (id, model name, norm, norm_amp_per_comp)
    ("pn-peak", "PhaseNet", "peak", True),
    ("pn-std", "PhaseNet", "std", True),
    ("eqt-std", "EQTransformer", "std", False),
    ("eqt-peak", "EQTransformer", "peak", False),
    ("eqt-percomp", "EQTransformer", "std", True),
]
IN_SAMPLES = {"PhaseNet": OC.PN_IN_SAMPLES, "EQTransformer": OC.EQT_IN_SAMPLES}


def gam(n):
    return n * U / (1.0 - n * U)


def effective(model_name, norm, per_comp):
    """(norm, per-channel amplitude?) as api.hip pre_args and SeisBench resolve them."""
    if model_name == "PhaseNet":
        return norm, True
    return ("peak", True) if per_comp else (norm, False)


def taper64(T):
    n = OC.EQT_TAPER_SAMPLES
    f = np.ones(T)
    tap = 0.5 * (1.0 + np.cos(np.linspace(np.pi, 2 * np.pi, n)))
    f[:n] *= tap
    f[-n:] *= tap[::-1]
    tapered = np.zeros(T, bool)
    tapered[:n] = tapered[-n:] = True
    return f, tapered


def pre64(x, model_name, norm, per_comp):
    """annotate_batch_pre of a raw (B, 3, T) float32 array in float64 -> (want, bound), both (B, 3, T) float64.

    |kernel - want| <= bound elementwise for any fp32 evaluation with the kernel's operation counts.  With dmu the error of the
    mean and damp that of the amplitude (module constants), d = x - mean, den = amp + eps, o = d / den:
    bound = [(dmu + U |d|) / den + |d| / den * damp / den] * taper + gam(C_OUT) |o * taper| + (tapered) C_TAP U |d| / den."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[1] == 3
    T = x.shape[2]
    norm, per = effective(model_name, norm, per_comp)
    x = x.astype(np.float64)
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    dmu = gam(C_MU) * np.abs(x).mean(-1, keepdims=True)
    dmu_a = dmu if per else dmu.max(1, keepdims=True)
    if norm == "peak":
        amp = np.abs(d).max(-1, keepdims=True)
        if not per:
            amp = amp.max(1, keepdims=True)
        damp = dmu_a + U * amp  # fmaxf(h - mu, mu - l): one rounding
    else:
        n = T if per else 3 * T
        amp = np.sqrt((d * d).sum(-1 if per else (-2, -1), keepdims=True) / (n - 1))
        # sum (d_i - e)^2 = S + n e^2 about a mean that is off by e: the std moves by at most |e| sqrt(n / (n - 1))
        damp = dmu_a * np.sqrt(n / (n - 1)) + gam(C_SS) * amp + STD_UNDERFLOW
    den = amp + OC.NORM_EPS
    o = d / den
    f, tapered = taper64(T) if model_name == "EQTransformer" else (np.ones(T), np.zeros(T, bool))
    want = o * f
    bound = ((dmu + U * np.abs(d)) / den + np.abs(o) * damp / den) * f + gam(C_OUT) * np.abs(want)
    bound = bound + tapered * (C_TAP * U) * np.abs(o)
    return want, bound


def pre_ratio(got, want, bound):
    """Largest |got - want| / bound; inf where got is not finite although want is."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got[np.isfinite(want)]).all():
        return np.inf
    err = np.abs(got - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def pre_inputs(T, seed, peak_only=False):
    """{name: (6, 3, T) float32}: the inputs on which a preprocessing kernel goes wrong.

    ``huge`` scales a window of unit peak by 1e15: the std kernels square in fp32, and 3 T * (2e15)^2 stays below the fp32
    maximum (3.4e38).  ``huge30`` (1e30) is for the peak configurations alone (``peak_only``): its squares overflow."""
    rng = np.random.default_rng(seed)
    plain = synthetic_windows(6, T, seed)
    unit = (plain / np.abs(plain).max((1, 2), keepdims=True)).astype(np.float32)
    out = {"plain": plain}
    out["counts+1e6"] = (np.round(unit * 2000.0) + 1e6).astype(np.float32)  # digitiser counts on a large offset
    c = plain.copy()
    c[:, 1] = 5.0  # a dead channel whose fp32 sums are exact
    c[:, 2] = np.float32(0.1) * np.float32(12345)  # and one whose sums are not
    out["constant"] = c
    s = plain.copy()
    for b in range(6):
        s[b, rng.integers(3), rng.integers(T)] = 1e9
    out["spike1e9"] = s
    out["tiny"] = (plain * np.float32(1e-30)).astype(np.float32)  # eps dominates the denominator
    out["huge"] = (unit * np.float32(1e15)).astype(np.float32)
    if peak_only:
        out["huge30"] = (unit * np.float32(1e30)).astype(np.float32)
    h = unit.copy()
    h[:, :, : T // 2] = 0.0
    h[:, 0] *= 1e4  # global against per-channel amplitude
    out["halfzero"] = h
    e = unit.copy()
    n = OC.EQT_TAPER_SAMPLES
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    e[:, :, :n] += 3.0 * sign * np.arange(1, n + 1, dtype=np.float32)  # energy under the taper, different at every sample
    e[:, :, -n:] -= 2.0 * sign * np.arange(2, n + 2, dtype=np.float32)
    out["edges"] = e
    for k, v in out.items():
        assert v.dtype == np.float32 and v.shape == (6, 3, T) and np.isfinite(v).all(), k
    return out


# ------------------------------------------------------------------------------------------------------------ stacking
def stack64(preds, starts, T, N, blind_l, blind_r, mode):
    """Blinding + overlap stacking of (n_windows, n_out, T) predictions as a scatter of counts and sums per output sample, in
    float64 -> (want (n_out, N), count (n_out, N), bound (n_out, N)).  NaN predictions are skipped, a sample nobody covers is
    NaN.  max is exact (bound 0).  avg: count - 1 additions, each of a partial sum of at most sum |v_i|, and one correctly
    rounded division: bound = U sum |v_i| = count U mean |v_i|."""
    preds = np.asarray(preds)
    n_out = preds.shape[1] if preds.ndim == 3 else 3
    cnt = np.zeros((n_out, N), np.int64)
    tot = np.zeros((n_out, N))
    mag = np.zeros((n_out, N))
    top = np.full((n_out, N), -np.inf)
    assert len(starts) == len(preds)
    for p, s in zip(preds, starts):
        s = int(s)
        assert 0 <= s and s + T <= N
        v = p[:, blind_l:T - blind_r].astype(np.float64)
        ok = ~np.isnan(v)
        sl = slice(s + blind_l, s + T - blind_r)
        cnt[:, sl] += ok
        tot[:, sl] += np.where(ok, v, 0.0)
        mag[:, sl] += np.where(ok, np.abs(v), 0.0)
        top[:, sl] = np.maximum(top[:, sl], np.where(ok, v, -np.inf))
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(cnt > 0, tot / cnt if mode == "avg" else top, np.nan)
    bound = U * mag if mode == "avg" else np.zeros_like(mag)
    return want, cnt, bound


def valid_range(starts, T, blind_l, blind_r):
    """(n_windows, first_valid, last_valid) that the windows and the blinding imply; (0, -1, -1) without a window."""
    if len(starts) == 0:
        return 0, -1, -1
    return len(starts), int(min(starts)) + blind_l, int(max(starts)) + T - blind_r - 1


def stack_ratio(got, want, bound):
    """(NaN pattern equal?, largest |got - want| / bound over the samples both hold; inf for a difference where bound is 0)."""
    got = np.asarray(got, np.float64)
    same = bool(np.array_equal(np.isnan(got), np.isnan(want)))
    both = ~np.isnan(got) & ~np.isnan(want)
    err = np.abs(got - want)[both]
    b = bound[both]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return same, float(r.max()) if r.size else 0.0


def STACK_CASES(T):
    """[(N, overlap, blind_l, blind_r, mode)] in the order the GPU test runs them on one handle: N and the blinding both shrink
    and grow from case to case.  The figures in the comments are for T = 3001; k() scales them to the window."""
    def k(v):
        return v * T // 3001

    half = k(1500)
    step = T - half
    dflt = {OC.PN_IN_SAMPLES: (OC.PN_DEFAULTS["overlap"],) + tuple(OC.PN_DEFAULTS["blinding"]),
            OC.EQT_IN_SAMPLES: (OC.EQT_DEFAULTS["overlap"],) + tuple(OC.EQT_DEFAULTS["blinding"])}.get(T, (half, 0, 0))
    mid = k(1500)
    return [
        (T, half, 0, 0, "avg"),                          # one window, no tail, count 1 everywhere
        (k(20000), k(1000), k(700), k(800), "max"),      # blinding wider than the overlap: NaN gaps inside the valid range
        (T + 1, half, 0, 0, "avg"),                      # the tail window one sample behind the only regular one
        (T + 7 * step, half, k(250), k(100), "avg"),     # N - T a multiple of the step: no tail window
        (T + 7 * step + 1, half, k(250), k(100), "avg"),         # ... + 1: a tail one sample behind the last regular window
        (T + 7 * step + step - 1, half, k(250), k(100), "avg"),  # ... + step - 1: a tail one sample short of a regular window
        (k(20000), 0, k(500), k(500), "avg"),            # no overlap, blinded: a gap at every window boundary
        (k(20000), 0, 0, 0, "avg"),                      # no overlap: count 1, the smaller blinding behind the larger one
        (k(9000), T - 11, 0, 0, "avg"),                  # step 11: up to 274 windows per sample
        (T + 299, T - 1, mid, T - 1 - mid, "avg"),       # step 1, one kept sample per window
        (T + 299, T - 1, 0, 0, "max"),                   # step 1, up to 300 windows per sample
        (k(60000),) + dflt + ("avg",),                   # the model's annotate defaults
        (k(45017), k(1777), 1, k(1222), "avg"),          # nothing round
        (T - 1, half, 0, 0, "avg"),                      # shorter than a window: no window, all NaN, first_valid = -1
        (k(20000), k(1000), 0, 0, "avg"),                # and back up behind the empty call
    ]


def stack_case_id(case):
    return "N{}-o{}-b{}_{}-{}".format(*case)

