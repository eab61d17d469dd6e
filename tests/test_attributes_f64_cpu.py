"""The attribute kernel's rule, plan and bounds without a GPU (tests/attributes_f64.py; volpick_amd/attributes.py's planner):
the restatement against literal scipy / numpy calls, the planned bins against fftfreq masks and the planned percentile
against np.percentile for every length up to the kernel's cap, the kernel's order of operations inside the frequency-index
bound against an extended-precision DFT -- and, in float32, far outside it -- and every NaN rule."""
import warnings

import numpy as np
import pytest
import scipy.fft
from scipy.signal import windows

from tests import attributes_f64 as A
from volpick_amd import attributes as VA

NAN = float("nan")


def _literal_fi(x, sr=100):
    n = len(x)
    spec = scipy.fft.fft(x * windows.hann(n))[0 : n // 2]
    freq = scipy.fft.fftfreq(n, 1.0 / sr)[0 : n // 2]
    up = np.mean(np.abs(spec)[np.logical_and(freq > 10, freq < 15)])
    low = np.mean(np.abs(spec)[np.logical_and(freq > 1, freq < 5)])
    return np.log10(up / low)


def test_restatement_matches_literal_calls():
    x = A.noise(4000, 1).astype(np.float64)
    p, s = 1000, 1700
    out, tol = A.trace_attributes(x, p, s)
    fis = [_literal_fi(x[c, 900:1600]) for c in range(3)]
    assert np.array_equal(out[A.OUT_FI], fis) and out[A.OUT_FI_TRACE] == np.mean(fis)
    noi = [np.percentile(np.abs(x[c, 500:1000]), 95) for c in range(3)]
    sig = [np.percentile(np.abs(x[c, 1700:2200]), 95) for c in range(3)]
    snr = [20 * np.log10(b / a) for a, b in zip(noi, sig)]
    assert np.array_equal(out[A.OUT_NOISE], noi) and np.array_equal(out[A.OUT_SIGNAL], sig)
    assert np.array_equal(out[A.OUT_SNR], snr) and out[A.OUT_SNR_MEAN] == np.nanmean(snr)
    assert (tol[A.OUT_NOISE] == 0).all() and (tol[A.OUT_SIGNAL] == 0).all() and (tol[A.OUT_FI] > 0).all()
    # S only as reference; no usable S -> the signal window follows P
    out2, _ = A.trace_attributes(x, NAN, 1700)
    assert out2[A.OUT_FI_TRACE] == np.mean([_literal_fi(x[c, 1600:2300]) for c in range(3)]) and np.isnan(out2[4:]).all()
    out3, _ = A.trace_attributes(x, 1000, 3990)
    assert np.array_equal(out3[A.OUT_SIGNAL], [np.percentile(np.abs(x[c, 1000:1500]), 95) for c in range(3)])
    out4, _ = A.trace_attributes(x, 1000, 3989)
    assert np.array_equal(out4[A.OUT_SIGNAL], [np.percentile(np.abs(x[c, 3989:4000]), 95) for c in range(3)])
    # demean: the span runs from the noise window's start to the frequency-index window's end
    xo = x + 1e4
    out5, tol5 = A.trace_attributes(xo, 1000, None, demean=True)
    xd = xo - xo[:, 500:1600].mean(axis=1, keepdims=True)
    assert np.array_equal(out5[A.OUT_NOISE], [np.percentile(np.abs(xd[c, 500:1000]), 95) for c in range(3)])
    assert out5[0] == _literal_fi(xd[0, 900:1600]) and (tol5[A.OUT_NOISE] > 0).all()


@pytest.mark.parametrize("sr", (100, 62.5))
def test_planned_bins_equal_fftfreq_masks_for_every_length(sr):
    for n in range(2, 2049):
        freq = scipy.fft.fftfreq(n, 1.0 / sr)[0 : n // 2]
        for band in (A.LOW_BAND, A.HIGH_BAND):
            mask = np.logical_and(freq > band[0], freq < band[1])
            first, count = VA.band_bins(n, sr, band)
            want = np.flatnonzero(mask)
            assert count == len(want), (n, band)
            if count:
                assert first == want[0] and np.array_equal(want, np.arange(first, first + count)), (n, band)


def test_bin_70_is_excluded_at_700_samples():
    freq = scipy.fft.fftfreq(700, 0.01)
    assert freq[70] == 10.0
    assert VA.band_bins(700, 100, A.LOW_BAND) == (8, 27) and VA.band_bins(700, 100, A.HIGH_BAND) == (71, 34)
    assert VA.band_bins(699, 100, A.LOW_BAND) == (7, 28) and VA.band_bins(699, 100, A.HIGH_BAND) == (70, 35)
    r = VA.plan_rows([4000], [1000], [NAN], 100)[0]
    assert (r["fi_start"], r["fi_n"], r["lo_first"], r["lo_count"], r["hi_first"], r["hi_count"]) == (900, 700, 8, 27, 71, 34)
    assert r["lo_count"] + r["hi_count"] == 61


def test_planned_percentile_equals_numpy_for_every_length():
    rng = np.random.default_rng(5)
    for m in range(1, 2049):
        a = np.abs(rng.standard_normal(m)) * 10.0 ** rng.uniform(-3, 3)
        if m % 7 == 0:
            a[rng.integers(0, m, m // 2)] = a[0]  # ties
        lo, up, g = VA.percentile_plan(m)
        assert 0 <= lo <= up <= min(lo + 1, m - 1) and 0.0 <= g < 1.0
        b = np.sort(a)
        d = b[up] - b[lo]
        got = b[up] - d * (1 - g) if g >= 0.5 else b[lo] + d * g
        assert got == np.percentile(a, 95), m
        if m <= 600 or m % 97 == 0 or m == 2048:
            assert A.emulate_percentile(a, lo, up, g) == np.percentile(a, 95), m


def test_percentile_with_nan_is_nan():
    a = np.array([1.0, NAN, 3.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(np.percentile(a, 95))
    assert np.isnan(A.emulate_percentile(a, *VA.percentile_plan(3)))


FI_CASES = [(n, dec, off) for n in (37, 101, 613, 699, 700, 2048) for dec in (-4.0, 0.0, 4.0) for off in (0.0, 1e4)]


@pytest.mark.parametrize("n,decades,offset", FI_CASES)
def test_kernel_order_is_inside_the_bound_and_float32_is_not(n, decades, offset):
    x = A.noise(n, 1000 + n, decades, offset)[0].astype(np.float64)
    bins = VA.band_bins(n, 100, A.LOW_BAND) + VA.band_bins(n, 100, A.HIGH_BAND)
    assert bins[1] > 0 and bins[3] > 0
    want, S, a_up, a_low = A.longdouble_fi(x, *bins)
    bound = A.fi_bound(n, S, a_up, a_low)
    r_scipy = abs(A.frequency_index(x, 0.01) - want) / bound
    r64 = abs(A.emulate_fi(x, *bins) - want) / bound
    r32 = abs(A.emulate_fi(x, *bins, dtype=np.float32) - want) / bound
    print(f"n={n} 1e{decades:+.0f} offset {offset:g}: scipy {r_scipy:.2e}, kernel order fp64 {r64:.2e}, fp32 {r32:.2e} of the bound")
    assert r_scipy <= 1.0 and r64 <= 1.0
    assert r32 > 1.0


def test_nan_rules():
    x = A.noise(4000, 2).astype(np.float64)
    rows = VA.plan_rows
    # neither onset; onsets that are sample 0
    for p, s in ((NAN, NAN), (None, None), (0, NAN), (0, 0)):
        out, _ = A.trace_attributes(x, p, s)
        assert np.isnan(out).all()
        r = rows([4000], [NAN if p is None else p], [NAN if s is None else s], 100)[0]
        assert r["fi_n"] == 0 and r["noise_n"] == 0 and r["signal_n"] == 0
    # P below 10: no SNR, the frequency index stands
    out, _ = A.trace_attributes(x, 9, NAN)
    assert np.isnan(out[4:]).all() and not np.isnan(out[:4]).any()
    out, _ = A.trace_attributes(x, 10, NAN)
    assert not np.isnan(out).any()
    assert rows([4000], [9], [NAN], 100)[0]["noise_n"] == 0 and rows([4000], [10], [NAN], 100)[0]["noise_n"] == 10
    # a band without a bin
    out, _ = A.trace_attributes(x, 3995, NAN)  # n = 105: both bands hold bins; n = 15 does not
    assert not np.isnan(out[:4]).any()
    out, _ = A.trace_attributes(x, 3995, NAN, fi_window=(0.1, 6.0))
    r = rows([4000], [3995], [NAN], 100, fi_window=(0.1, 6.0))[0]
    assert r["fi_n"] == 15 and r["lo_count"] == 0 and np.isnan(out[:4]).all()
    # flat components are skipped; all flat -> NaN
    y = x.copy()
    y[1] = 3.0
    out, _ = A.trace_attributes(y, 1000, NAN)
    assert np.isnan(out[1]) and out[A.OUT_FI_TRACE] == np.mean([out[0], out[2]])
    out, _ = A.trace_attributes(np.ones((3, 4000)), 1000, NAN)
    assert np.isnan(out[:4]).all()
    # zeros -> isclose -> NaN for that component, nanmean over the rest
    y = x.copy()
    y[2, 500:1000] = 0.0
    out, _ = A.trace_attributes(y, 1000, NAN)
    assert np.isnan(out[12]) and out[6] == 0.0 and out[A.OUT_SNR_MEAN] == np.mean(out[10:12])
    # a NaN sample: in the FI window only, in the noise window only
    y = x.copy()
    y[0, 1200] = NAN
    out, _ = A.trace_attributes(y, 1000, 2000)
    assert np.isnan(out[0]) and out[A.OUT_FI_TRACE] == np.mean(out[1:3]) and not np.isnan(out[4:]).any()
    y = x.copy()
    y[0, 600] = NAN
    out, _ = A.trace_attributes(y, 1000, 2000)
    assert np.isnan(out[4]) and np.isnan(out[10]) and not np.isnan(out[[5, 6, 7, 8, 9, 11, 12, 13]]).any()
    assert not np.isnan(out[:4]).any()  # a NaN outside the FI window: the dead-component sum is NaN, which is not <= 1e-9


def test_planned_windows_equal_the_restatement_for_random_onsets():
    rng = np.random.default_rng(11)
    n_rows = 4000
    N = rng.integers(1, 7000, n_rows)
    p = np.where(rng.random(n_rows) < 0.2, NAN, rng.integers(-50, 7200, n_rows) + rng.random(n_rows))
    s = np.where(rng.random(n_rows) < 0.3, NAN, rng.integers(0, 7200, n_rows) + rng.random(n_rows))
    p[:40], s[:40] = rng.integers(0, 12, 40), np.where(rng.random(40) < 0.5, NAN, 0.0)
    for kw in ({}, {"fi_window": (0.5, 2.25), "snr_window": 1.37}):
        rows = VA.plan_rows(N, p, s, 100, **kw)
        for i in range(n_rows):
            w = A.windows_of(N[i], p[i], s[i], 100, **kw)
            r = rows[i]
            for name, key in (("fi", "fi"), ("noise", "noise"), ("signal", "signal")):
                want = w[name] if w[name] is not None and w[name][1] > w[name][0] else None
                got = (int(r[key + "_start"]), int(r[key + "_start"]) + int(r[key + "_n"])) if r[key + "_n"] else None
                if name != "fi" and w["noise"] is not None and want is None:
                    continue  # an empty SNR window beside a planned one: both sides answer NaN for it
                assert got == want, (i, name, N[i], p[i], s[i])
