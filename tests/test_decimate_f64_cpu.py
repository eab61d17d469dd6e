"""What gives the bound of tests/decimate_f64.py its teeth, without a GPU: the kernel's scheme emulated in float64 passes it,
the same scheme in float32 or with too short a warm-up does not; and the host path the device path is measured against has not
moved: same coefficients to the last bit, same ``resample_array`` results as before the coefficient helper was factored out."""
import numpy as np
import pytest

from tests.decimate_f64 import FACTORS, N_LONG, RATE_OUT, bound, counts, emulate, ratio, want64, warmup
from volpick_amd.resample import lowpass_sos, resample_array


@pytest.mark.parametrize("k", FACTORS)
def test_chunked_float64_emulation_is_within_the_bound(k):
    x = counts(N_LONG, 100 + k)
    want = want64(x, k)
    assert want.shape == ((N_LONG + k - 1) // k,)
    r = ratio(emulate(x, k), want, x)
    print(f"k={k}: worst |emulation - want| / bound = {r:.4f}")
    assert r <= 1.0
    # pieces as short as one thread's (32 samples), warm-up from the pole radius: still the reference's own rounding
    assert ratio(emulate(x[:50_001], k, chunk=32), want64(x[:50_001], k), x[:50_001]) <= 1.0


def test_rounding_the_answer_itself_uses_a_quarter_of_the_bound():
    x = counts(N_LONG, 110)
    want = want64(x, 10)
    r = ratio(want.astype(np.float32), want, x)
    assert 0.1 < r <= 0.25 * 1.3 + 1e-9  # 2^-24 |y| <= 2^-24 * 1.3 max|x| against 2^-22 max|x|


def test_float32_state_breaks_the_bound():
    x = counts(N_LONG, 110)
    r = ratio(emulate(x, 10, dtype=np.float32), want64(x, 10), x)
    print(f"float32 coefficients and state, k=10: {r:.2f} x bound")
    assert r > 4.0


@pytest.mark.parametrize("k", (2, 10))
def test_short_warmup_breaks_the_bound(k):
    x = counts(N_LONG, 100 + k)
    assert ratio(emulate(x, k, warm=8), want64(x, k), x) > 100.0


def test_warmup_lengths_from_the_pole_radius():
    got = {k: warmup(lowpass_sos(RATE_OUT * 0.5, RATE_OUT * k)) for k in (2, 5, 10, 20, 40)}
    assert got[2] == 69 and got[5] == 122 and got[10] == 234
    assert got[20] < got[40] <= 1024  # what the kernel's tile has room for


def test_edges_of_the_emulation_are_the_whole_trace_filter():
    # shorter than any warm-up, and a few samples around a chunk seam
    for n in (1, 7, 50, 4095, 4096, 4097):
        x = counts(n, n)
        for k in (2, 5, 20):
            assert ratio(emulate(x, k), want64(x, k), x) <= 1.0


@pytest.mark.parametrize("k", (2, 4, 5, 10, 20, 40))
def test_coefficient_helper_returns_what_lowpass_zerophase_used(k):
    from scipy.signal import iirfilter, zpk2sos

    df = RATE_OUT * k
    z, p, g = iirfilter(4, (RATE_OUT * 0.5) / (0.5 * df), btype="lowpass", ftype="butter", output="zpk")
    want = zpk2sos(z, p, g)
    got = lowpass_sos(RATE_OUT * 0.5, df)
    assert got.dtype == np.float64 and got.shape == (2, 6)
    assert got.tobytes() == want.tobytes()
    assert (got[:, 3] == 1.0).all()


def test_resample_array_results_have_not_moved():
    """Values computed with volpick_amd/resample.py as it was before ``lowpass_sos`` was factored out."""
    rng = np.random.default_rng(2024)
    x = np.round(800 * rng.standard_normal(20011) + 123456.0)
    table = {
        200.0: (10006, 1235204642.514137, [93481.50993612217, 131574.71743299876, 123796.64578037238, 11547.58243416716]),
        500.0: (4003, 494021074.3516658, [74677.83629068494, 131906.17446584208, 123936.04880062431, 594.1324956404178]),
    }
    for rate, (n, total, samples) in table.items():
        y = resample_array(x, rate, 100.0)
        assert y.dtype == np.float64 and len(y) == n
        np.testing.assert_allclose(y[[0, 1, n // 2, -1]], samples, rtol=1e-13, atol=0)
        np.testing.assert_allclose(float(y.sum()), total, rtol=1e-13, atol=0)
    y = resample_array(x[:5000], 250.0, 100.0)  # the Fourier branch, untouched
    assert len(y) == 2000
    np.testing.assert_allclose([float(y.sum()), float(y[1234])], [246911056.0, 123968.47105868199], rtol=1e-12, atol=0)
    assert bound(x) > 0
