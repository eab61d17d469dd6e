"""Inputs, the float64 answer and the bound that the CPU and GPU tests of the device Fourier resampler share
(volpick_amd/csrc/fourier.hip, ``vp_resample_fourier``).  Numpy and scipy only; nothing here touches the device code.

Answer: ``want64(x, rate) = resample_fourier(x.astype(float64), rate, 100.0)`` from the product's own host module -- the path
every such trace took before the kernel existed, and the restatement of ObsPy's ``Trace.resample(window="hann")``.

Bound, on every output sample: ``|got - want| <= 2^-22 max|x|``.  With float64 arithmetic the only error left is the final
rounding to float32, at most 2^-24 |y|; max|y| / max|x| is 0.99 on this data at N = 400 003 (the Hann window only attenuates, and
linear interpolation of the spectrum does not overshoot); rounding ``want`` itself to float32 gives 0.21 of the bound, so the
bound leaves the same factor 4.8 over the reference's own rounding as the decimation bound does.  float64 rounding noise of the
chirp-z scheme (``emulate`` below) does not show at that scale.  No constant here was taken from a run of the kernel.

``emulate`` restates the kernel's scheme: both DFTs as Bluestein convolutions with the chirp phase reduced in integers, over
power-of-two FFTs cut into the kernel's passes (``fft_passes``), each pass followed by its twiddle, the inverse FFT running the
passes backwards from the permuted order the forward FFT leaves."""
import numpy as np

from tests.decimate_f64 import KINDS, counts  # noqa: F401  (shared inputs)
from volpick_amd.resample import resample_fourier

RATE_OUT = 100.0
RATES = (250, 125, 80, 66, 50, 40, 20)
N_LONG = 400_003
LOG_TILE = 12
FFT_TILE = 1 << LOG_TILE  # the largest transform the kernel does inside LDS (TILE in fourier.hip)
FFT_COLS = 16  # adjacent columns a strided pass takes at least (1 << LOG_COLS): bounds a strided pass at FFT_TILE / FFT_COLS points
PASS_LIMITS = (FFT_TILE, FFT_TILE * (FFT_TILE // FFT_COLS))  # largest M done in one pass, in two passes
MAX_M = 1 << 27


def want64(x, rate):
    return resample_fourier(np.asarray(x, dtype=np.float64), float(rate), RATE_OUT)


def host_args(n, rate_in, rate_out=RATE_OUT):
    """num, df, d_large_f exactly as resample_fourier forms them."""
    factor = rate_in / float(rate_out)
    num = int(n / factor)
    df = 1.0 / (n * (1.0 / rate_in))
    d_large_f = 1.0 / num * rate_out if num else float("nan")
    return num, df, d_large_f


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


def fft_size(length):
    """log2 of the FFT a Bluestein convolution of `length` points runs over: the least M = 2^k >= 2 length - 1."""
    k = 0
    while (1 << k) < 2 * length - 1:
        k += 1
    return k


def fft_passes(logm):
    """[(logP, logS)]: the kernel's passes for M = 2^logm -- P points at stride S, the last pass contiguous."""
    if logm <= LOG_TILE:
        logp = [logm]
    else:
        r = logm - LOG_TILE
        logp = [r] if (1 << logm) <= PASS_LIMITS[1] else [(r + 1) // 2, r // 2]
        logp.append(LOG_TILE)
    out, logs = [], logm
    for p in logp:
        logs -= p
        out.append((p, logs))
    return out


def length_for_passes(npass, side):
    """The Bluestein length on either side of a pass-count switch: the longest still done in `npass` passes (side 0) and the
    shortest that takes one more (side 1)."""
    m = PASS_LIMITS[npass - 1]
    return m // 2 + side  # 2 L - 1 <= M  <=>  L <= M / 2


def _twiddle(p, s, sign):
    k = np.arange(p, dtype=np.int64)[:, None]
    c = np.arange(s, dtype=np.int64)[None, :]
    return np.exp(sign * 2j * np.pi * ((k * c) / float(p * s)))


def _fft_forward(a, passes):
    m = len(a)
    for logp, logs in passes:
        p, s = 1 << logp, 1 << logs
        v = np.fft.fft(a.reshape(m // (p * s), p, s), axis=1)
        if s > 1:
            v = v * _twiddle(p, s, -1.0)
        a = v.reshape(m)
    return a  # in the passes' permuted order


def _fft_inverse(a, passes):
    m = len(a)
    for logp, logs in reversed(passes):
        p, s = 1 << logp, 1 << logs
        v = a.reshape(m // (p * s), p, s)
        if s > 1:
            v = v * _twiddle(p, s, 1.0)
        a = (np.fft.ifft(v, axis=1) * p).reshape(m)
    return a  # natural order, not yet divided by M


def chirp(j, length, sign, mode="int"):
    """exp(sign i pi j^2 / length).  mode "int": the phase reduced in integers, as the kernel does; "float64" / "float32": the
    phase formed as pi j j / length in that format without reduction (what the kernel must not do)."""
    if mode == "int":
        r = (j.astype(np.int64) * j.astype(np.int64)) % (2 * length)
        ph = np.pi * (r / float(length))
        return np.cos(ph) + 1j * sign * np.sin(ph)
    t = np.dtype(mode).type
    jf = j.astype(t)
    ph = (t(np.pi) * jf * jf / t(length)).astype(t)
    return (np.cos(ph) + 1j * sign * np.sin(ph)).astype(np.complex128)


def bluestein(v, length, sign, mode="int"):
    """DFT of `length` points with exponent sign `sign` of v (zero beyond len(v)), all `length` outputs."""
    logm = fft_size(length)
    m, passes = 1 << logm, fft_passes(logm)
    j = np.arange(length, dtype=np.int64)
    c = chirp(j, length, sign, mode)
    a = np.zeros(m, dtype=np.complex128)
    a[: len(v)] = v * c[: len(v)]
    b = np.zeros(m, dtype=np.complex128)
    b[:length] = np.conj(c)
    if length > 1:
        b[m - length + 1:] = np.conj(c[1:][::-1])
    spec = _fft_forward(a, passes) * _fft_forward(b, passes) * (1.0 / m)
    return _fft_inverse(spec, passes)[:length] * c


def emulate(x, rate_in, rate_out=RATE_OUT, mode="int"):
    """The kernel's scheme on the host, float64 throughout, one rounding to float32 at the end."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    num, df, d_large_f = host_args(n, float(rate_in), float(rate_out))
    spec = bluestein(x, n, -1.0, mode)[: n // 2 + 1]
    spec.imag[0] = 0.0
    if n % 2 == 0:
        spec.imag[-1] = 0.0
    if n > 1:
        jw = (np.arange(n // 2 + 1, dtype=np.int64) + n // 2) % n
        spec = spec * (0.5 - 0.5 * np.cos(np.pi * ((2 * jw) / float(n))))
    f = df * np.arange(0, n // 2 + 1, dtype=np.int32)
    large_f = d_large_f * np.arange(0, num // 2 + 1, dtype=np.int32)
    half = np.interp(large_f, f, spec.real) + 1j * np.interp(large_f, f, spec.imag)
    half.imag[0] = 0.0
    if num % 2 == 0:
        half.imag[-1] = 0.0
    full = np.empty(num, dtype=np.complex128)  # Hermitian extension
    full[: num // 2 + 1] = half
    if num > 1:
        mm = np.arange(num // 2 + 1, num)
        full[mm] = np.conj(half[num - mm])
    y = bluestein(full, num, 1.0, mode).real / float(n)
    return y.astype(np.float32)
