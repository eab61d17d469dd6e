"""Filtering and detrending through the public surface, on the device: ``Trace.filter`` / ``Trace.detrend`` of device-resident
streams, and the ``filter_args`` / ``filter_kwargs`` of a model inside ``annotate``.  On the parent commit ``Trace.filter`` does
not exist and the model arguments are swallowed, so every test here fails there.

Bound (tests/sosfilt_f64.py): ``2^-22 max|x|`` on every sample.  A chain of k device steps rounds to float32 k times, each time
by at most 2^-24 of that step's output; after the first detrend the outputs stay below 0.3 max|x| (the offset is gone), so the
four steps of the reference's chain together stay below 4 * 2^-24 * 0.3 * 1.2 max|x| = 0.36 of the bound."""
import numpy as np
import pytest

from tests import sosfilt_f64 as S
from volpick_amd.synthetic import synthetic_stream_array

pytestmark = pytest.mark.gpu

N = 30_000


def _host_stream(rate=100.0, n=N, seed=77):
    """Three components of counts: events and noise on a strong 0.15 Hz microseism on a large offset."""
    import volpick_amd as va

    data, _, _ = synthetic_stream_array(n, seed=seed, n_events=4)
    t = np.arange(n) / rate
    swell = 3.0 * np.sin(2 * np.pi * 0.15 * t)
    t0 = va.UTCDateTime("2022-02-03T04:05:06")
    st = va.Stream()
    for c, comp in enumerate("ZNE"):
        cnt = np.round((data[c] + swell * (1.0 + 0.2 * c)) * 2.0e4 + 123456.0).astype(np.int32)
        st.append(va.Trace(cnt, dict(network="XX", station="FLT", location="", channel="HH" + comp, starttime=t0, sampling_rate=rate)))
    return st


def _reference_chain(st):  # volpick/data/utils.py:675-704, as written there
    st.detrend("demean").detrend("linear")
    st.filter("highpass", freq=0.3)
    return st.filter("bandpass", freqmin=1, freqmax=20)


def test_reference_chain_on_a_device_stream_stays_there_and_matches_the_host():
    import volpick_amd as va

    host = _host_stream()
    raw = [tr.data.astype(np.float64) for tr in host]
    dev = va.to_device(host)
    assert _reference_chain(dev) is dev
    _reference_chain(host)
    for tr, ref, x in zip(dev, host, raw):
        assert tr._dev is not None and tr._dev.is_cuda and tr._data is None and tr.stats.npts == N
        assert str(tr._dev.dtype) == "torch.float32" and ref.data.dtype == np.float64
        r = S.ratio(tr._dev.cpu().numpy(), ref.data, x)
        print(f"{tr.id}: reference chain on the device vs host, worst / bound = {r:.4f}")
        assert r <= 1.0
        assert tr._data is None  # the comparison went through _dev, not through .data


def _filtered_model(**kw):
    from volpick_amd import PhaseNet

    plain = PhaseNet.from_pretrained("volpick")
    model = PhaseNet(norm=plain.norm, component_order=plain.component_order, phases=plain.labels, **kw)
    model.load_state_dict(plain.state_dict())
    model.default_args = dict(plain.default_args)
    return plain.cuda(), model.cuda()


def _rows(out):
    return {tr.stats.channel: (tr.stats.starttime, np.asarray(tr.data)) for tr in out}


def test_model_filter_args_filter_inside_annotate_and_leave_the_callers_traces_alone():
    import torch

    import volpick_amd as va

    plain, model = _filtered_model(filter_args=("highpass",), filter_kwargs={"freq": 0.3})
    assert model.filter_args == ("highpass",) and model.filter_kwargs == {"freq": 0.3}
    raw = va.to_device(_host_stream())
    before = [(tr._dev, tr._dev.clone()) for tr in raw]
    got = _rows(model.annotate(raw))
    for tr, (d, copy) in zip(raw, before):  # copy=True: never modified, never copied to the host
        assert tr._dev is d and tr._data is None and torch.equal(d, copy) and str(d.dtype) == "torch.int32"
    pre = va.to_device(_host_stream()).filter("highpass", freq=0.3)
    assert all(tr._data is None for tr in pre)
    want = _rows(plain.annotate(pre))
    unfiltered = _rows(plain.annotate(raw))
    assert set(got) == set(want) == set(unfiltered) and len(got) == 3
    for ch in got:
        assert got[ch][0] == want[ch][0] and got[ch][1].shape == want[ch][1].shape
        assert np.array_equal(got[ch][1].view(np.uint32), want[ch][1].view(np.uint32))  # the same bits
        delta = float(np.abs(got[ch][1] - unfiltered[ch][1]).max())
        print(f"{ch}: filtered vs unfiltered annotation, max |delta| = {delta:.3e}")
        assert delta > 1e-3  # the microseism is gone: a different picture
    # copy=False filters the caller's traces in place, as upstream does -- still on the device
    inplace = _rows(model.annotate(raw, copy=False))
    for tr, p in zip(raw, pre):
        assert tr._data is None and str(tr._dev.dtype) == "torch.float32" and torch.equal(tr._dev, p._dev)
    assert all(np.array_equal(inplace[ch][1], got[ch][1]) for ch in got)


def test_a_200_hz_device_trace_is_filtered_at_200_hz_then_decimated():
    import torch

    import volpick_amd as va
    from volpick_amd import models
    from volpick_amd.resample import decimate_device, resample_array
    from volpick_amd.signal import butter_sos, filter_array, sos_filter_device

    assert models.FILTER_BEFORE_RESAMPLE
    fast = va.to_device(_host_stream(rate=200.0, n=2 * N))
    flt = (("highpass",), {"freq": 0.3})
    groups = list(models._group_stream(fast, "ZNE", 100.0, True, 3001, flt))
    assert len(groups) == 1
    block = groups[0]["data"]
    assert torch.is_tensor(block) and block.is_cuda and tuple(block.shape) == (3, N)
    order = {tr.stats.channel[-1]: tr for tr in fast}
    sos200 = butter_sos("highpass", 200.0, freq=0.3)
    for c, comp in enumerate("ZNE"):
        tr = order[comp]
        assert tr.stats.sampling_rate == 200.0 and tr.stats.npts == 2 * N and tr._data is None and str(tr._dev.dtype) == "torch.int32"
        assert torch.equal(block[c], decimate_device(sos_filter_device(tr._dev, sos200), 200.0, 100.0))
        # and the host's order of the same two steps, within two roundings passed through a gain below 1.3: under the bound
        x = tr._dev.cpu().numpy().astype(np.float64)
        host = resample_array(filter_array(x, "highpass", 200.0, freq=0.3), 200.0, 100.0)
        r = S.ratio(block[c].cpu().numpy(), host, x)
        print(f"{tr.id}: filter at 200 Hz, then decimate: device vs host, worst / bound = {r:.4f}")
        assert r <= 1.0
        # the other order is a different filter: its corner sits at another fraction of the rate
        other = sos_filter_device(decimate_device(tr._dev, 200.0, 100.0), butter_sos("highpass", 100.0, freq=0.3))
        assert not torch.equal(other, block[c])
    plain, model = _filtered_model(filter_args=flt[0], filter_kwargs=flt[1])
    got = _rows(model.annotate(fast))
    want = _rows(plain.annotate(va.to_device(_host_stream(rate=200.0, n=2 * N)).filter("highpass", freq=0.3)))
    assert len(got) == 3 and all(np.array_equal(got[ch][1], want[ch][1]) for ch in got)


def test_a_refused_filter_warns_with_the_trace_id_and_takes_the_host_path():
    import volpick_amd as va
    from volpick_amd.signal import filter_array

    host = _host_stream()
    x = host[0].data.astype(np.float64)
    tr = va.to_device(host)[0]
    with pytest.warns(UserWarning, match=r"XX\.FLT\.\.HHZ: filtering on the device refused .*n_sections = 6"):
        assert tr.filter("bandpass", freqmin=1, freqmax=20, corners=6) is tr  # six sections: beyond the kernel's four
    assert tr._dev is None and tr.data.dtype == np.float64
    assert np.array_equal(tr.data, filter_array(x, "bandpass", 100.0, freqmin=1, freqmax=20, corners=6))
