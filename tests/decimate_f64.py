"""Inputs, the float64 answer and the bound that the CPU and GPU tests of the device decimation share
(volpick_amd/csrc/resample.hip, ``vp_decimate_lowpass``).  Numpy and scipy only; nothing here touches the device code.

Answer: ``want = lowpass_zerophase(x.astype(float64), rate_out / 2, rate_in)[::k]`` from the product's own host module -- the
path every trace took before the kernel existed, and the restatement of SeisBench's rule.

Bound, on every output sample: ``|got - want| <= 2^-22 max|x|``.  With float64 state and intermediate the only error left is the
final rounding to float32, at most 2^-24 |y|; a Butterworth low-pass has gain <= 1 and its step overshoot keeps max|y| within about
1.3 max|x|; truncating the warm-up at r^W <= 2^-40 and float64 rounding noise are far below.  The chunked float64 emulation below
gives 0.84 * 2^-24 max|x| (what rounding ``want`` itself to float32 gives), so the bound leaves a factor 4.8 over the reference's
own rounding.  No constant here was taken from a run of the kernel."""
import numpy as np

from volpick_amd.resample import lowpass_sos, lowpass_zerophase

RATE_OUT = 100.0
FACTORS = (2, 4, 5, 10, 20)
N_LONG = 400_003  # a multiple of no factor and of no tile
TILE = 8192  # samples per workgroup of the kernel (DT * DC in resample.hip): the seams the edge cases sit on
KINDS = {"int32": (0, np.int32), "float32": (1, np.float32), "float64": (2, np.float64)}  # VP_SAMPLES_* and numpy dtype


def counts(n, seed):
    """Seismic counts: noise on a slow swing on a large offset, as integers held in float64 (exact in int32 and float32 too)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    return np.round(800.0 * rng.standard_normal(n) + 30000.0 * np.sin(i / 5000.0) + 123456.0)


def want64(x, k):
    return lowpass_zerophase(np.asarray(x, dtype=np.float64), RATE_OUT * 0.5, RATE_OUT * k)[::k]


def bound(x):
    return 2.0 ** -22 * float(np.abs(np.asarray(x, dtype=np.float64)).max())


def ratio(got, want, x):
    """Worst |got - want| / bound over every sample (inf where the shapes or a NaN disagree)."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float("inf")
    b = bound(x)
    d = float(np.abs(got - want).max()) if got.size else 0.0
    return d / b if b > 0 else (0.0 if d == 0 else float("inf"))


def pole_radius(sos):
    r = 0.0
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos, dtype=np.float64):
        r = max(r, float(np.abs(np.roots([a0, a1, a2])).max()))
    return r


def warmup(sos):
    """Samples after which the response to a wrong starting state has decayed by 2^-40: r^W <= 2^-40."""
    return int(np.ceil(40.0 * np.log(2.0) / -np.log(pole_radius(sos))))


def emulate(x, k, chunk=4096, warm=None, dtype=np.float64):
    """The kernel's scheme on the host: both passes cut into chunks, every chunk but those at the start of a pass run from
    zero state ``warm`` samples ahead of itself (default: from the pole radius); arithmetic in ``dtype``; the kept samples
    rounded to float32 at the end."""
    from scipy.signal import sosfilt

    sos = lowpass_sos(RATE_OUT * 0.5, RATE_OUT * k).astype(dtype)
    warm = warmup(sos.astype(np.float64)) if warm is None else warm

    def one_pass(u):
        out = np.empty(len(u), dtype=dtype)
        for c0 in range(0, len(u), chunk):
            c1 = min(c0 + chunk, len(u))
            s = max(0, c0 - warm)
            y = sosfilt(sos, u[s:c1])
            assert y.dtype == dtype
            out[c0:c1] = y[c0 - s:]
        return out

    f = one_pass(np.asarray(x, dtype=dtype))
    g = one_pass(f[::-1])[::-1]
    return g[::k].astype(np.float32)
