"""What gives the bound of tests/fourier_f64.py its teeth, without a GPU: the kernel's scheme (Bluestein over power-of-two FFTs
cut into the kernel's passes, chirp phase reduced in integers) emulated in float64 passes it at every rate and at the short
lengths; the same scheme with a single-precision phase does not; and the host path the device path is measured against has
not moved.

Measured here and asserted below (N = 400 003, worst |emulation - want| / bound over the seven rates):
  integer-reduced phase       0.2091 .. 0.2096   -- exactly what rounding ``want`` itself to float32 gives
  pi * j * j / L in float64   0.2096 .. 0.2103   -- worse, but inside the bound: at this length j^2 / L reaches 4e5 turns, a
                                                    float64 phase keeps ~1e-10 of a radian, and the bound is 2.4e-7 relative
  pi * j * j / L in float32   4.9e5 .. 9.2e5     -- far outside
So the bound catches a single-precision phase; an unreduced float64 phase it does not catch at this length, and the test below
asserts what is true of it instead: its chirp is wrong by more than a thousand float64 roundings where the reduced one is
within a few, which is why the kernel reduces in integers (a component-day has 54 times the samples)."""
import numpy as np
import pytest

from tests.fourier_f64 import (FFT_TILE, N_LONG, PASS_LIMITS, RATES, bound, chirp, counts, emulate, fft_passes, fft_size,
                               host_args, length_for_passes, ratio, want64)
from volpick_amd.resample import fourier_args, resample_array


@pytest.mark.parametrize("rate", RATES)
def test_emulation_is_within_the_bound_at_every_rate(rate):
    x = counts(N_LONG, 100 + rate)
    want = want64(x, rate)
    assert want.shape == (host_args(N_LONG, float(rate))[0],)
    r = ratio(emulate(x, rate), want, x)
    r_self = ratio(want.astype(np.float32), want, x)
    print(f"{rate} -> 100 Hz: worst |emulation - want| / bound = {r:.4f}; rounding want itself: {r_self:.4f}; "
          f"max|y| / max|x| = {np.abs(want).max() / np.abs(x).max():.4f}")
    assert r <= 1.0
    assert 0.15 < r_self <= 0.25 + 1e-9  # 2^-24 |y| with max|y| <= max|x|, against 2^-22 max|x|
    assert np.abs(want).max() <= np.abs(x).max()


@pytest.mark.parametrize("n", (1, 2, 3, 7, 50))
def test_emulation_is_within_the_bound_at_short_lengths(n):
    ran = 0
    for rate in RATES:
        if host_args(n, float(rate))[0] < 1:  # N = 1: the upsampling rates only
            continue
        x = counts(n, 7 * n + rate)
        r = ratio(emulate(x, rate), want64(x, rate), x)
        print(f"n={n} {rate} Hz: {r:.4f}")
        assert r <= 1.0
        ran += 1
    assert ran >= 3


@pytest.mark.parametrize("n", (5000, 5001, 4999, 5004))
def test_emulation_parities_and_pass_seams(n):
    for rate in (250, 125, 50):
        x = counts(n, 11 * n + rate)
        assert ratio(emulate(x, rate), want64(x, rate), x) <= 1.0
    for side in (0, 1):  # either side of the one-pass / two-pass switch, as the forward transform's length
        m = length_for_passes(1, side)
        x = counts(m, m)
        assert ratio(emulate(x, 250), want64(x, 250), x) <= 1.0


def test_pass_structure():
    assert PASS_LIMITS == (FFT_TILE, FFT_TILE * FFT_TILE // 16)
    assert [len(fft_passes(k)) for k in (0, 1, 12, 13, 20, 21, 27)] == [1, 1, 1, 2, 2, 3, 3]
    for k in range(28):
        ps = fft_passes(k)
        assert sum(p for p, _ in ps) == k and ps[-1][1] == 0
        for i, (p, s) in enumerate(ps[:-1]):  # a strided pass: at least 16 adjacent columns of a full tile
            assert 12 - p >= 4 and s == sum(q for q, _ in ps[i + 1:])
    assert fft_size(1) == 0 and fft_size(2) == 2 and fft_size(2048) == 12 and fft_size(2049) == 13
    assert fft_size(8_640_000) == 25 and fft_size(21_600_000) == 26


def test_single_precision_chirp_phase_breaks_the_bound():
    x = counts(N_LONG, 350)
    want = want64(x, 250)
    r = ratio(emulate(x, 250, mode="float32"), want, x)
    print(f"chirp phase pi j j / L in float32, N = {N_LONG}: {r:.3g} x bound")
    assert r > 1000.0


def test_unreduced_float64_chirp_phase_is_a_thousand_roundings_off():
    x = counts(N_LONG, 350)
    want = want64(x, 250)
    r_int, r_f64 = ratio(emulate(x, 250), want, x), ratio(emulate(x, 250, mode="float64"), want, x)
    print(f"chirp phase pi j j / L in float64 without reduction, N = {N_LONG}: {r_f64:.4f} x bound (reduced: {r_int:.4f})")
    assert r_f64 > r_int  # measurably worse, though inside the bound at this length (module docstring)
    j = np.arange(N_LONG, dtype=np.int64)
    exact = chirp(j, N_LONG, -1.0)
    # the reduced phase against the same reduction carried out in extended precision
    ph = ((j * j) % (2 * N_LONG)).astype(np.longdouble) / np.longdouble(N_LONG) * np.longdouble(np.pi)
    ref = np.cos(ph) - 1j * np.sin(ph)
    err_int = float(np.abs(exact - ref).max())
    err_f64 = float(np.abs(chirp(j, N_LONG, -1.0, mode="float64") - ref).max())
    print(f"worst chirp error: reduced {err_int:.2e}, unreduced float64 {err_f64:.2e}")
    assert err_int < 8 * 2.0 ** -53 and err_f64 > 1000 * 2.0 ** -53


def test_host_arguments_are_the_host_functions_own():
    for n in (1, 7, 4_319_999, 21_600_000):
        for rate in RATES:
            num, df, dlf = host_args(n, float(rate))
            if num < 1:
                continue
            got = fourier_args(n, float(rate), 100.0)
            assert got[0] == num and got[1].hex() == df.hex() and got[2].hex() == dlf.hex()


def test_resample_array_results_have_not_moved():
    """Values computed with volpick_amd/resample.py as it was before the device path existed, on the input
    tests/test_decimate_f64_cpu.py pins."""
    rng = np.random.default_rng(2024)
    x = np.round(800 * rng.standard_normal(20011) + 123456.0)
    table = {
        250.0: (8004, 988174059.899851, [123875.84511465127, 123742.38535824514, 123937.39731715825, 122918.19559928357]),
        50.0: (40022, 4941117219.554202, [123995.04231939572, 124388.82904121294, 123986.66050525579, 123493.000013988]),
        40.0: (50027, 6176334794.429016, [123995.03650604162, 124325.89920911801, 124012.06124375844, 123593.75830326973]),
    }
    for rate, (n, total, samples) in table.items():
        y = resample_array(x, rate, 100.0)
        assert y.dtype == np.float64 and len(y) == n
        np.testing.assert_allclose(y[[0, 1, n // 2, -1]], samples, rtol=1e-13, atol=0)
        np.testing.assert_allclose(float(y.sum()), total, rtol=1e-13, atol=0)
    assert bound(x) > 0


@pytest.mark.parametrize("poison", (np.nan, np.inf))
@pytest.mark.parametrize("rate", (250.0, 40.0))
def test_host_answer_to_a_nonfinite_sample_is_nan_everywhere(poison, rate):
    x = counts(5001, 5)
    x[2500] = poison
    for dtype in (np.float64, np.float32):
        y = resample_array(x.astype(dtype), rate, 100.0)
        assert len(y) == host_args(5001, rate)[0] and np.isnan(y).all()
