"""The teeth of the bound the device filter is held to (tests/sosfilt_f64.py), and the host side of filtering and detrending:
no GPU.

1. the float64 emulation of the carry scheme, rounded to float32, stays within ``2^-22 max|x|`` for the whole filter set, one-pass
and zero-phase, at every seam length; 2. each of the ways the scheme can go wrong exceeds it: the warm-up scheme of the
decimation kernel (1024-sample halo) on the 0.3 Hz high-pass, float32 state, a carry dropped at tile seams, a carry dropped at
piece seams; 3. ``butter_sos``: bit-equal to ``lowpass_sos``, ObsPy's Nyquist rules; 4. host ``Trace.filter`` / ``detrend``
equal the direct scipy composition and chain; 5. ``filter_args`` / ``filter_kwargs`` survive ``save`` then ``load``."""
import warnings

import numpy as np
import pytest

from tests import sosfilt_f64 as S
from volpick_amd.resample import lowpass_sos
from volpick_amd.signal import butter_sos, detrend_array, filter_array


@pytest.mark.parametrize("name", list(S.FILTERS))
def test_float64_carry_scheme_stays_within_the_bound(name):
    sos = S.sos_of(name)
    assert len(sos) <= 4
    for zerophase in (False, True):
        for n in S.LENGTHS:
            x = S.trace(n)
            w = S.want(name, n, zerophase)
            r_round = S.ratio(w.astype(np.float32), w, x)
            r = S.ratio(S.emulate(x, sos, zerophase), w, x)
            print(f"{name} zerophase={zerophase} n={n}: max|y|/max|x| = {np.abs(w).max() / np.abs(x).max():.3f}, "
                  f"float32(want) {r_round:.4f}, emulation {r:.4f}")
            assert r <= 1.0


def test_first_order_section_is_in_the_set():
    sos = S.sos_of("highpass 1 Hz, 3 corners")
    assert any(row[2] == 0.0 and row[5] == 0.0 for row in sos)
    assert len(S.sos_of("highpass 1 Hz, 2 corners")) == 1 and len(S.sos_of("bandpass 1-20 Hz")) == 4


def test_the_ways_the_scheme_can_go_wrong_exceed_the_bound():
    n = 40_003
    x = S.trace(n)
    hp = "highpass 0.3 Hz"
    r = S.ratio(S.emulate_warmup(x, S.sos_of(hp)), S.want(hp, n, False), x)
    print(f"warm-up scheme, 1024 halo, {hp}: {r:.1f} x the bound")
    assert r > 100.0
    for name in S.FILTERS:
        sos = S.sos_of(name)
        w = S.want(name, n, False)
        r32 = S.ratio(S.emulate(x, sos, dtype=np.float32), w, x)
        r_tile = S.ratio(S.emulate(x, sos, carry="no_tile"), w, x)
        r_piece = S.ratio(S.emulate(x, sos, carry="no_piece"), w, x)
        print(f"{name}: float32 state {r32:.1f}, no carry at tile seams {r_tile:.1f}, none at piece seams {r_piece:.1f}")
        assert r_tile > 1.0 and r_piece > 1.0
        if name != "lowpass 20 Hz":  # (its memory is a few samples: single precision costs it about the bound, no more)
            assert r32 > 10.0


def test_butter_sos_is_lowpass_sos_and_keeps_the_nyquist_rules():
    for freq, df, corners in ((50.0, 200.0, 4), (20.0, 100.0, 4), (5.0, 100.0, 3)):
        assert np.array_equal(butter_sos("lowpass", df, corners=corners, freq=freq), lowpass_sos(freq, df, corners))
    def outcome(call):  # what scipy makes of a corner AT Nyquist is scipy's business (recent versions refuse it)
        try:
            return call()
        except ValueError as e:
            return str(e)

    with pytest.warns(UserWarning, match="above Nyquist"):
        clamped = outcome(lambda: butter_sos("lowpass", 100.0, freq=60.0))
    with pytest.warns(UserWarning, match="above Nyquist"):
        assert np.array_equal(clamped, outcome(lambda: lowpass_sos(60.0, 100.0)))
    with pytest.warns(UserWarning, match="high-pass instead"):
        bp = butter_sos("bandpass", 100.0, freqmin=1.0, freqmax=50.0)
    assert np.array_equal(bp, butter_sos("highpass", 100.0, freq=1.0))
    with pytest.raises(ValueError, match="above Nyquist"):
        butter_sos("highpass", 100.0, freq=51.0)
    with pytest.raises(ValueError, match="above Nyquist"), pytest.warns(UserWarning, match="Setting Nyquist"):
        butter_sos("bandstop", 100.0, freqmin=51.0, freqmax=60.0)
    with pytest.warns(UserWarning, match="Setting Nyquist"):
        outcome(lambda: butter_sos("bandstop", 100.0, freqmin=10.0, freqmax=60.0))
    with pytest.raises(ValueError):
        butter_sos("chebyshev", 100.0, freq=1.0)
    assert butter_sos("bandpass", 100.0, freqmin=1.0, freqmax=20.0).shape == (4, 6)


def test_host_trace_filter_and_detrend_are_the_scipy_composition():
    from scipy.signal import detrend, iirfilter, sosfilt, zpk2sos

    import volpick_amd as va

    x = S.counts(5003, 3)
    hdr = dict(network="XX", station="A", channel="HHZ", sampling_rate=100.0)
    st = va.Stream([va.Trace(x.astype(np.int32), hdr), va.Trace(x.astype(np.float32), dict(hdr, channel="HHN"))])
    # the reference's chain (volpick/data/utils.py:675-704) works as written and returns the stream
    out = st.detrend("demean").detrend("linear").filter("highpass", freq=0.3)
    assert out is st
    assert st.filter("bandpass", freqmin=1, freqmax=20, zerophase=True) is st
    y = detrend(detrend(x, type="constant"), type="linear")
    y = sosfilt(zpk2sos(*iirfilter(4, 0.3 / 50.0, btype="highpass", ftype="butter", output="zpk")), y)
    sos = zpk2sos(*iirfilter(4, [1 / 50.0, 20 / 50.0], btype="band", ftype="butter", output="zpk"))
    y = sosfilt(sos, sosfilt(sos, y)[::-1])[::-1]
    for tr in st:
        assert tr.data.dtype == np.float64 and tr.stats.npts == 5003 and np.array_equal(tr.data, y)
    tr = va.Trace(x.copy(), hdr)
    assert tr.detrend() is tr  # ObsPy's default: the line through the first and last sample
    assert np.array_equal(tr.data, x - (x[0] + np.arange(5003) * (x[-1] - x[0]) / 5002.0))
    assert tr.data[0] == 0.0 and tr.data[-1] == 0.0
    assert np.array_equal(detrend_array(x, "constant"), detrend_array(x, "demean"))
    assert np.array_equal(filter_array(x.astype(np.int32), "lowpass", 100.0, freq=20.0), sosfilt(lowpass_sos(20.0, 100.0), x))
    masked = va.Trace(x, hdr)
    masked._data = np.ma.masked_array(x, mask=x > 1e9)  # what a gappy merge leaves in an ObsPy trace
    with pytest.raises(NotImplementedError, match="split the stream at its gaps first"):
        masked.filter("highpass", freq=1.0)
    with pytest.raises(NotImplementedError, match="split the stream at its gaps first"):
        masked.detrend("linear")
    with pytest.raises(ValueError):
        va.Trace(x[:1], hdr).detrend("linear")


def test_filter_args_survive_save_and_load(tmp_path, lib):
    import json

    from volpick_amd import EQTransformer, PhaseNet

    plain = PhaseNet.from_pretrained("volpick")
    assert plain.filter_args is None and plain.filter_kwargs is None
    assert "filter_args" not in plain.get_model_args() and "filter_kwargs" not in plain.get_model_args()
    model = PhaseNet(filter_args=("highpass",), filter_kwargs={"freq": 0.3, "zerophase": True})
    model.load_state_dict(plain.state_dict())
    model.save(tmp_path / "filtered")
    meta = json.loads((tmp_path / "filtered.json").read_text())
    assert meta["model_args"]["filter_args"] == ["highpass"]
    assert meta["model_args"]["filter_kwargs"] == {"freq": 0.3, "zerophase": True}
    back = PhaseNet.load(tmp_path / "filtered")
    assert back.filter_args == ("highpass",) and back.filter_kwargs == {"freq": 0.3, "zerophase": True}
    assert back.get_model_args() == model.get_model_args()
    eqt = EQTransformer(filter_args=["bandpass"], filter_kwargs=dict(freqmin=1, freqmax=20))
    assert eqt.filter_args == ("bandpass",) and eqt.get_model_args()["filter_kwargs"] == dict(freqmin=1, freqmax=20)
