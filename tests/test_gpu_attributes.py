"""The attribute kernel (volpick_amd/csrc/attributes.hip) against the float64 restatement and its derived bounds
(tests/attributes_f64.py; their teeth: tests/test_attributes_f64_cpu.py), through the C ABI (``vp_attributes``,
``vp_bank_attributes``) and the public surface (``bank_attributes``, ``pick_attributes``).

1. one (3, 4000) float32 array with an offset of 1e4, every edge of the rule as a row of ONE launch (clipped windows, odd /
even / prime n, an empty band, p = 9 / 10, s = N - 10 / N - 11, noise windows of 1, 2, 499 samples, ties, zeros, a NaN in one
window only, with and without demean, both caps), two more arrays for dead components, and the 2049-sample argument error;
2. a bank of six traces of unequal length; 3. the same launch twice, and into device memory, gives identical bits; 4. a
stream with a 2 Hz and a 12 Hz burst, classified, device-resident and on the host; 5. a pick that matches no block.

Every case prints its figure (worst |got - want| / bound over the row's 14 values; 0 = equal, percentiles of rows without
demean must be equal bit for bit) before it asserts; LOG.md, "Frequency index and SNR on the device", says which of them
have been measured on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import attributes_f64 as A
from volpick_amd import _lib
from volpick_amd import attributes as VA

pytestmark = pytest.mark.gpu

VP_ERR_INVALID = -1
N = 4000
NAN = float("nan")


def _array():
    """Clean noise around 1e4 in [0, 2500) and [2950, 4000); between them one NaN (component 0, sample 2500), a run of zeros
    (component 2, [2600, 2700)) and a run of heavily tied values (component 1, [2750, 2950))."""
    x = A.noise(N, 77, 2.0, 1e4)
    x[0, 2500] = np.nan
    x[2, 2600:2700] = 0.0
    x[1, 2750:2950] = 1e4 + 64.0 * np.round((x[1, 2750:2950] - 1e4) / 64.0)
    return x


# name -> (p, s, planner arguments)
CASES = {
    "interior, P and S": (1000, 1600, {}),
    "interior, P only": (1000, NAN, {}),
    "interior, S only (no SNR)": (NAN, 1600, {}),
    "neither onset": (NAN, NAN, {}),
    "P = 0 is falsy, S is the reference": (0, 1300, {}),
    "ref < wb, even n = 650": (50, NAN, {}),
    "ref < wb, odd n = 637": (37, 400, {}),
    "p = 9": (9, NAN, {}),
    "p = 10": (10, NAN, {}),
    "ref + wa > N, n = 400": (3700, NAN, {}),
    "ref + wa > N, prime n = 499": (3601, NAN, {}),
    "n = 700 (bin 70 excluded)": (1500, NAN, {}),
    "n = 699": (3401, NAN, {}),
    "a band is empty (n = 15)": (3995, NAN, {"fi_window": (0.1, 6.0)}),
    "s = N - 10 (signal behind P)": (3500, N - 10, {}),
    "s = N - 11 (signal behind S)": (3500, N - 11, {}),
    "noise window of 1 sample": (1200, NAN, {"snr_window": 0.01}),
    "noise window of 2 samples": (1200, NAN, {"snr_window": 0.02}),
    "noise window of 499 samples": (499, NAN, {}),
    "ties in the noise window": (2950, NAN, {"snr_window": 2.0}),
    "zeros in the noise window (isclose)": (2700, NAN, {"snr_window": 1.0}),
    "NaN in the FI window only": (1950, NAN, {}),
    "NaN in the noise window only": (2990, NAN, {}),
    "FI window at the cap of 2048": (1200, NAN, {"fi_window": (10.24, 10.24)}),
    "noise window at the cap of 2048": (2100, NAN, {"snr_window": 20.48}),
    "other bands": (1000, 1600, {"low_band": (0.5, 3), "high_band": (20, 40)}),
}
DEMEAN = ("interior, P and S", "interior, P only", "ref < wb, even n = 650", "ref < wb, odd n = 637", "p = 10",
          "ref + wa > N, n = 400", "ref + wa > N, prime n = 499", "n = 700 (bin 70 excluded)", "n = 699",
          "s = N - 10 (signal behind P)", "s = N - 11 (signal behind S)", "noise window of 1 sample",
          "noise window of 2 samples", "noise window of 499 samples", "ties in the noise window",
          "NaN in the FI window only", "NaN in the noise window only", "FI window at the cap of 2048",
          "noise window at the cap of 2048", "interior, S only (no SNR)", "a band is empty (n = 15)", "other bands")
ALL_CASES = [(name, False) for name in CASES] + [(name, True) for name in DEMEAN]


def _plan(cases, n=N):
    rows = np.concatenate([VA.plan_rows([n], [CASES[name][0]], [CASES[name][1]], 100, demean=dm, **CASES[name][2])
                           for name, dm in cases])
    rows["trace"] = 0
    return rows


def _launch(x_dev, rows, out=None):
    """vp_attributes on a (3, n) CUDA tensor -> (return code, (n_rows, 14) host array); `out`: a CUDA float64 tensor instead."""
    host = np.full((len(rows), 14), -7.0)
    ptr = C.c_void_p(out.data_ptr()) if out is not None else host.ctypes.data_as(C.c_void_p)
    rc = _lib.load().vp_attributes(0, C.c_void_p(x_dev.data_ptr()), x_dev.shape[1], rows.ctypes.data_as(C.POINTER(_lib.VpAttrRow)),
                                   len(rows), ptr, None)
    return rc, (out.cpu().numpy() if out is not None else host)


@functools.lru_cache(maxsize=None)
def _main_launch():
    import torch

    x = _array()
    rows = _plan(ALL_CASES)
    rc, got = _launch(torch.from_numpy(x).cuda(), rows)
    _lib.check(rc, "vp_attributes")
    want = {}
    for name, dm in ALL_CASES:
        p, s, kw = CASES[name]
        want[name, dm] = A.trace_attributes(x, p, s, demean=dm, **kw)
    got.setflags(write=False)
    return x, rows, got, want


def test_the_launch_holds_about_48_rows_and_every_kind_of_window():
    _, rows, _, _ = _main_launch()
    assert len(rows) == len(ALL_CASES) == 48
    assert {499, 637, 650, 699, 700, 2048, 15, 400} <= set(rows["fi_n"].tolist())
    assert {1, 2, 10, 499, 500, 2048} <= set(rows["noise_n"].tolist()) and 11 in rows["signal_n"].tolist()
    assert (rows["lo_count"][rows["fi_n"] == 15] == 0).all()


@pytest.mark.parametrize("name,demean", ALL_CASES)
def test_every_edge_of_the_rule_in_one_launch(name, demean):
    _, _, got, want = _main_launch()
    i = ALL_CASES.index((name, demean))
    w, tol = want[name, demean]
    r = A.ratio(got[i], w, tol)
    print(f"{name}{' (demean)' if demean else ''}: worst |got - want| / bound = {r:.3e}; fi {got[i][3]:.6f} snr {got[i][13]:.6f}")
    assert r <= 1.0
    if not demean:  # percentiles of rows without demean: numpy's, bit for bit
        assert np.array_equal(got[i][4:10], w[4:10], equal_nan=True)


def test_the_cases_reach_the_branches_they_name():
    _, _, got, want = _main_launch()
    g = {k: got[i] for i, k in enumerate(ALL_CASES)}
    assert np.isnan(g["neither onset", False]).all()
    assert np.isnan(g["p = 9", False][4:]).all() and not np.isnan(g["p = 9", False][:4]).any()
    assert not np.isnan(g["p = 10", False]).any()
    assert np.isnan(g["a band is empty (n = 15)", False][:4]).all() and not np.isnan(g["a band is empty (n = 15)", False][4:]).any()
    z = g["zeros in the noise window (isclose)", False]
    assert z[6] == 0.0 and np.isnan(z[12]) and not np.isnan(z[[10, 11, 13]]).any()
    f = g["NaN in the FI window only", False]
    assert np.isnan(f[0]) and not np.isnan(f[1:]).any()
    m = g["NaN in the noise window only", False]
    assert np.isnan(m[[4, 10]]).all() and not np.isnan(m[[0, 1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13]]).any()
    assert not np.array_equal(g["s = N - 10 (signal behind P)", False][7:10], g["s = N - 11 (signal behind S)", False][7:10])
    # without demean the offset of 1e4 drowns every percentile; with it the ratio is that of the noise
    assert abs(g["interior, P only", False][13]) < 0.2 and np.isfinite(g["interior, P only", True][13])


@pytest.mark.parametrize("which", ("one component flat", "all components flat"))
def test_dead_components_are_skipped(which):
    import torch

    x = A.noise(N, 78, 1.0, 0.0)
    x[1] = 3.0
    if which == "all components flat":
        x[0], x[2] = -2.0, 0.0
    cases = [("interior, P and S", False), ("interior, P and S", True), ("ref + wa > N, n = 400", False)]
    rc, got = _launch(torch.from_numpy(x).cuda(), _plan(cases))
    _lib.check(rc, "vp_attributes")
    for i, (name, dm) in enumerate(cases):
        w, tol = A.trace_attributes(x, CASES[name][0], CASES[name][1], demean=dm)
        r = A.ratio(got[i], w, tol)
        print(f"{which}, {name}{' (demean)' if dm else ''}: worst |got - want| / bound = {r:.3e}")
        assert r <= 1.0
        assert np.isnan(got[i][1]) and np.isnan(got[i][3]) == (which == "all components flat")


@pytest.mark.parametrize("kw", ({"fi_window": (10.24, 10.25)}, {"snr_window": 20.49}))
def test_a_window_of_2049_samples_is_an_argument_error(kw):
    import torch

    x = torch.from_numpy(A.noise(N + 400, 79)).cuda()
    good = VA.plan_rows([N + 400], [2100], [NAN], 100)
    bad = VA.plan_rows([N + 400], [2100], [NAN], 100, **kw)
    assert max(bad[0]["fi_n"], bad[0]["noise_n"]) == 2049
    rows = np.concatenate([good, bad])
    rows["trace"] = 0
    rc, got = _launch(x, rows)
    msg = _lib.last_error()
    print(f"2049 samples: rc = {rc}, message = {msg!r}")
    assert rc == VP_ERR_INVALID and "2049" in msg and "row 1" in msg
    assert (got == -7.0).all()  # nothing written
    dev = torch.full((2, 14), -7.0, dtype=torch.float64, device="cuda")
    rc, got = _launch(x, rows, out=dev)
    assert rc == VP_ERR_INVALID and (got == -7.0).all()
    # a window outside the trace, an unknown flag and a bin past n / 2 are refused as well
    for field, value in (("fi_start", N), ("flags", 2), ("hi_count", 400), ("noise_up", 600)):
        rows = good.copy()
        rows[field] = value
        rc, got = _launch(x, rows)
        assert rc == VP_ERR_INVALID and (got == -7.0).all(), field


# ------------------------------------------------------------------------------------------ the bank
BANK = ((37, 20, NAN), (101, NAN, 50), (700, NAN, NAN), (1500, 400.7, 900.2), (3001, 1500, 2995), (6000, 3000, NAN))


def test_bank_of_six_traces_of_unequal_length():
    from volpick_amd.generate import WaveformBank

    traces = [A.noise(n, 300 + n, 1.0) for n, _, _ in BANK]
    bank = WaveformBank(traces, {"P": np.array([p for _, p, _ in BANK]), "S": np.array([s for _, _, s in BANK])})
    try:
        got = VA.bank_attributes(bank, raw=True)
        cols = VA.bank_attributes(bank)
    finally:
        bank.close()
    assert got.shape == (6, 14)
    for i, (n, p, s) in enumerate(BANK):
        w, tol = A.trace_attributes(traces[i], p, s)
        r = A.ratio(got[i], w, tol)
        print(f"bank trace of {n} samples (P {p}, S {s}): worst |got - want| / bound = {r:.3e}")
        assert r <= 1.0
        assert np.array_equal(got[i][4:10], w[4:10], equal_nan=True)
    assert np.isnan(got[2]).all() and np.isnan(got[1][4:]).all() and not np.isnan(got[[0, 3, 4, 5]]).any()
    assert set(cols) == set(VA.COLUMNS)
    assert cols["trace_frequency_index"].shape == (6,) and cols["trace_snr_db"].shape == (6, 3)
    assert cols["trace_mean_snr_db"].shape == (6,) and cols["component_frequency_index"].shape == (6, 3)
    assert np.array_equal(cols["trace_frequency_index"], got[:, 3], equal_nan=True)
    assert np.array_equal(cols["trace_snr_db"], got[:, 10:13], equal_nan=True)


# ------------------------------------------------------------------------------------------ determinism
def test_the_same_launch_twice_and_into_device_memory_gives_identical_bits():
    import torch

    x, rows, first, _ = _main_launch()
    d = torch.from_numpy(x).cuda()
    rc, again = _launch(d, rows)
    _lib.check(rc, "vp_attributes")
    dev = torch.full((len(rows), 14), -7.0, dtype=torch.float64, device="cuda")
    rc, on_device = _launch(d, rows, out=dev)
    _lib.check(rc, "vp_attributes")
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    assert np.array_equal(first.view(np.uint64), on_device.view(np.uint64))


# ------------------------------------------------------------------------------------------ end to end
N_STREAM, LP_AT, VT_AT = 12_000, 3000, 8000


@functools.lru_cache(maxsize=None)
def _burst_stream():
    """100 Hz counts with an offset: noise, a 2 Hz burst at 30 s and a 12 Hz burst at 80 s on all three components."""
    import volpick_amd as va

    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, N_STREAM)) * 20.0 + 5000.0
    t = np.arange(1500) / 100.0
    env = np.exp(-t / 1.5) * 2000.0
    for at, hz in ((LP_AT, 2.0), (VT_AT, 12.0)):
        for c, a in enumerate((1.0, 0.6, 0.5)):
            x[c, at : at + 1500] += a * env * np.sin(2 * np.pi * hz * t)
    x = x.astype(np.float32)
    t0 = va.UTCDateTime("2020-01-01T00:00:00")
    st = va.Stream([va.Trace(x[c].copy(), {"network": "XX", "station": "BRST", "location": "", "channel": "HH" + comp,
                                           "starttime": t0, "sampling_rate": 100.0}) for c, comp in enumerate("ZNE")])
    x.setflags(write=False)
    return st, x, t0


def test_picks_of_a_classified_stream_device_resident_and_on_the_host():
    import volpick_amd as va

    st, x, t0 = _burst_stream()
    model = va.PhaseNet.from_pretrained("volpick").cuda()
    picks = list(model.classify(st).picks)
    # the two onsets themselves, whether or not the picker found them
    picks += [va.Pick("XX.BRST.", t0 + LP_AT / 100.0, peak_time=t0 + LP_AT / 100.0, phase="P"),
              va.Pick("XX.BRST.", t0 + VT_AT / 100.0, peak_time=t0 + VT_AT / 100.0, phase="P")]
    moved = va.to_device(st)
    on_host = va.pick_attributes(st, picks, raw=True)
    on_device = va.pick_attributes(moved, picks, raw=True)
    assert all(tr._dev is not None and tr._data is None for tr in moved)  # never copied back
    assert on_host.shape == (len(picks), 14)
    assert np.array_equal(on_host.view(np.uint64), on_device.view(np.uint64))
    worst = 0.0
    for i, pk in enumerate(picks):
        k = int(round((pk.peak_time - t0) * 100.0))
        w, tol = A.trace_attributes(x, k, None, demean=True)
        r = A.ratio(on_host[i], w, tol)
        print(f"pick {i} ({pk.phase} at sample {k}): worst |got - want| / bound = {r:.3e}; fi {on_host[i][3]:.4f} snr {on_host[i][13]:.2f}")
        worst = max(worst, r)
    assert worst <= 1.0
    cols = va.pick_attributes(moved, picks)
    fi_lp, fi_vt = cols["trace_frequency_index"][-2:]
    want_lp = A.trace_attributes(x, LP_AT, None, demean=True)[0][3]
    want_vt = A.trace_attributes(x, VT_AT, None, demean=True)[0][3]
    print(f"{len(picks) - 2} picks from classify; FI of the 2 Hz burst {fi_lp:.4f} (restatement {want_lp:.4f}), of the 12 Hz burst "
          f"{fi_vt:.4f} ({want_vt:.4f}); mean SNR {cols['trace_mean_snr_db'][-2]:.2f}, {cols['trace_mean_snr_db'][-1]:.2f} dB")
    assert want_lp < want_vt and fi_lp < fi_vt
    assert want_lp < -1.0 and want_vt > 0.5 and cols["trace_mean_snr_db"][-1] > 20.0


def test_a_pick_that_matches_no_block_is_a_nan_row():
    import volpick_amd as va

    st, x, t0 = _burst_stream()
    picks = [va.Pick("XX.BRST.", t0 + 30.0, peak_time=t0 + 30.0, phase="P"),
             va.Pick("ZZ.NONE.", t0 + 30.0, peak_time=t0 + 30.0, phase="P"),
             va.Pick("XX.BRST.", t0 + 500.0, peak_time=t0 + 500.0, phase="S"),  # the right station, outside its block
             va.Pick("XX.BRST.", t0 + 80.0, peak_time=None, phase="S")]
    cols = va.pick_attributes(st, picks)
    assert not np.isnan(cols["trace_frequency_index"][0]) and not np.isnan(cols["trace_snr_db"][0]).any()
    for k in VA.COLUMNS:
        assert np.isnan(cols[k][1:]).all(), k
    empty = va.pick_attributes(st, [])
    assert empty["trace_frequency_index"].shape == (0,) and empty["trace_snr_db"].shape == (0, 3)
