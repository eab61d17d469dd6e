"""GPU: what the Python trace layer promises and the per-operation tests leave to chance -- every field of what ``read`` /
``read_mseed`` / ``read_many`` return for each combination of ``device_resident`` and ``dtype``; that a trace operation on a
device-backed trace is the direct ``*_device`` call bit for bit and leaves the trace on the device with its header right;
the full text of a refusal's warning and the host answer behind it; and the one upload rule of ``to_device`` and
``Trace.spectrogram``.

Every refusal here is an argument check of the library that returns before any launch.  Traces hold 1,000 to 5,000 samples,
with one exception: ``Trace.trigger`` clips its windows to the trace's length, so ``nlta`` beyond the kernel's 65,536 samples
needs a trace that long."""
import functools
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

import volpick_amd as va
from oracle import mseed as OM
from tests.mseed_util import T0, file_bytes, seismogram
from tests.stalta_f64 import MAX_NLTA
from volpick_amd import _lib
from volpick_amd import io as vio
from volpick_amd import resample as RS
from volpick_amd import signal as SG
from volpick_amd import spectrogram as SP
from volpick_amd import trigger as TR
from volpick_amd.stream import UTCDateTime

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "bench_steim2_6min.mseed"


# ------------------------------------------------------------------------------------------------------- reading files
@functools.lru_cache(maxsize=None)
def _files():
    rng = np.random.default_rng(23)
    hdr = dict(network="XX", station="LAY", location="", rate=100.0, start_us=T0)
    text = np.frombuffer(b"2020-09-13 12:26:40 clock locked; mass centred; door opened\r\n" * 4, np.uint8).astype(np.int32)
    return {
        "golden": GOLDEN.read_bytes(),
        "steim2": file_bytes([dict(hdr, channel="HHZ", data=seismogram(3000, rng))]),
        "float32": file_bytes([dict(hdr, channel="HHE", data=rng.standard_normal(1200).astype(np.float32))], encoding=4),
        "text": file_bytes([dict(hdr, channel="LOG", rate=1.0, data=text)], encoding=0),
        "mixed": (file_bytes([dict(hdr, channel="HHZ", data=seismogram(2500, rng))])
                  + file_bytes([dict(hdr, channel="HHN", data=rng.standard_normal(1100).astype(np.float32))], encoding=4)),
    }


IDS = {"golden": ["XX.VOLC..HHE", "XX.VOLC..HHN", "XX.VOLC..HHZ"], "steim2": ["XX.LAY..HHZ"], "float32": ["XX.LAY..HHE"],
       "text": ["XX.LAY..LOG"], "mixed": ["XX.LAY..HHN", "XX.LAY..HHZ"]}


@functools.lru_cache(maxsize=None)
def _expected(name):
    """Per trace of the file, in order: (header dict as ``read`` must give it, the oracle's samples, encoding).  Every
    channel of these files is one continuous segment, so a trace's records are the records of its channel."""
    buf = _files()[name]
    recs, out = OM.scan_records(buf), []
    for w in OM.read_mseed(buf):
        rs = [r for r in recs if r["channel"] == w["channel"]]
        assert sum(r["nsamples"] for r in rs) == len(w["data"])
        mseed = dict(dataquality="D", format_version=2, publication_version=None, number_of_records=len(rs),
                     encoding=rs[0]["encoding"], byteorder=">" if rs[0]["big_endian"] else "<", record_length=rs[0]["reclen"],
                     steim_integrity_errors=0)
        stats = dict(network=w["network"], station=w["station"], location=w["location"], channel=w["channel"],
                     starttime=UTCDateTime._from_us(w["start_us"]), sampling_rate=float(w["rate"]), npts=len(w["data"]),
                     mseed=mseed, _format="MSEED")
        out.append((stats, w["data"], rs[0]["encoding"]))
    return out


def _read(route, buf, **kw):
    if route == "read":
        return vio.read(buf, **kw)
    if route == "read_mseed":
        return vio.read_mseed(buf, **kw)
    streams = vio.read_many([_files()["steim2"], buf, _files()["float32"]], **kw)
    assert len(streams) == 3 and [tr.id for tr in streams[0]] == IDS["steim2"] and [tr.id for tr in streams[2]] == IDS["float32"]
    return streams[1]


@pytest.mark.parametrize("route", ["read", "read_mseed", "many"])
@pytest.mark.parametrize("dtype", [None, np.float32], ids=["own", "f32"])
@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(IDS))
def test_every_field_of_what_reading_returns(name, resident, dtype, route):
    st = _read(route, _files()[name], dtype=dtype, device_resident=resident)
    want = _expected(name)
    assert isinstance(st, va.Stream) and [tr.id for tr in st] == IDS[name] and len(want) == len(IDS[name])
    for tr, (stats, x, enc) in zip(st, want):
        assert dict(tr.stats) == stats and set(tr.stats) == set(stats)
        if dtype is not None:
            x = x.astype(dtype)
        elif enc == 0 and not resident:
            x = x.astype(np.uint8).view("S1")
        if resident:
            assert tr._data is None and tr._dev.is_cuda and tr._dev.dim() == 1
            got = tr._dev.cpu().numpy()
        else:
            assert tr._dev is None
            got = tr.data
        assert got.dtype == x.dtype and got.shape == x.shape and got.tobytes() == x.tobytes()


def test_defaults_of_device_resident():
    buf = _files()["steim2"]
    assert vio.read_mseed(buf)[0]._dev is None and vio.read(buf)[0]._dev is None
    assert vio.read_many([buf])[0][0]._dev.is_cuda


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
def test_a_short_payload_is_named_by_its_offset_in_its_own_file(resident):
    rng = np.random.default_rng(29)
    good = file_bytes([dict(network="XX", station="BAD", location="", channel="HHZ", rate=100.0, start_us=T0,
                            data=seismogram(300, rng))], encoding=3)  # 112 samples a record
    bad = bytearray(good)
    bad[512 + 30: 512 + 32] = (900).to_bytes(2, "big")  # record 1 claims more samples than its payload holds
    text = "miniSEED record at byte 512: payload holds fewer samples than its header says"
    for call in (lambda: vio.read_mseed(bytes(bad), device_resident=resident),
                 lambda: vio.read(bytes(bad), device_resident=resident),
                 lambda: vio.read_many([_files()["steim2"], bytes(bad), good], device_resident=resident)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


# ------------------------------------------------------------------------------------------------------------ the step
HDR = dict(network="XX", station="T", location="", channel="HHZ", starttime=UTCDateTime(T0 / 1e6))


def _samples(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 100.0
    return (2000.0 + 30.0 * t + 400.0 * np.sin(2 * np.pi * 3.0 * t) + 60.0 * rng.standard_normal(n).cumsum()).astype(np.float32)


def _pair(rate, x=None):
    """(device-backed trace, its host twin, the samples)."""
    x = _samples() if x is None else x
    hdr = dict(HDR, sampling_rate=rate)
    return va.to_device(va.Stream([va.Trace(x.copy(), hdr)]))[0], va.Trace(x.copy(), hdr), x


def _bits(t):
    return t.cpu().numpy().tobytes()


def _on_device_f32(tr, n, rate):
    import torch

    assert tr._data is None and tr._dev.is_cuda and tr._dev.dtype == torch.float32 and tuple(tr._dev.shape) == (n,)
    assert tr.stats.npts == n == len(tr) and tr.stats.sampling_rate == rate
    assert tr.stats.starttime == HDR["starttime"] and tr.id == "XX.T..HHZ"


def _on_host(tr, want, rate):
    assert tr._dev is None and tr.data.dtype == want.dtype and tr.data.tobytes() == want.tobytes()
    assert tr.stats.npts == len(want) and tr.stats.sampling_rate == rate


def _in_place_ops():
    import torch

    sos = SG.butter_sos("bandpass", 100.0, freqmin=1, freqmax=20)
    return {
        "filter": (lambda tr: tr.filter("bandpass", freqmin=1, freqmax=20), lambda d: SG.sos_filter_device(d, sos, False),
                   lambda x: SG.filter_array(x, "bandpass", 100.0, freqmin=1, freqmax=20)),
        "detrend": (lambda tr: tr.detrend("linear"), lambda d: SG.detrend_device(d, "linear"),
                    lambda x: SG.detrend_array(x, "linear")),
        "trigger": (lambda tr: tr.trigger("recstalta", sta=0.5, lta=5.0),
                    lambda d: TR.sta_lta_device(d, "recstalta", 50, 500, torch.float32),
                    lambda x: TR.recursive_sta_lta(x, 50, 500)),
    }


@pytest.mark.parametrize("op", ["filter", "detrend", "trigger"])
def test_an_in_place_step_is_the_direct_device_call_and_stays_on_the_device(op):
    method, direct, host_fn = _in_place_ops()[op]
    dev, host, x = _pair(100.0)
    before = dev._dev
    want = direct(before)
    assert method(dev) is dev
    _on_device_f32(dev, len(x), 100.0)
    assert dev._dev is not before and _bits(dev._dev) == _bits(want)
    assert _bits(before) == x.tobytes()  # the step wrote a new tensor
    assert method(host) is host
    _on_host(host, host_fn(x), 100.0)
    assert host.data.dtype == np.float64


RESAMPLE = {"integer": (200.0, lambda d: RS.decimate_device(d, 200.0, 100.0)),
            "fourier": (250.0, lambda d: RS.fourier_device(d, 250.0, 100.0))}


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "in_place"])
@pytest.mark.parametrize("ratio", sorted(RESAMPLE))
def test_resample_is_the_direct_device_call_and_honours_copy(ratio, copy):
    rate, direct = RESAMPLE[ratio]
    dev, host, x = _pair(rate)
    before, ptr = dev._dev, dev._dev.data_ptr()
    want = direct(before)
    out = RS.resample_trace(dev, 100.0, copy=copy, fourier_on_device=True)
    _on_device_f32(out, int(want.shape[0]), 100.0)
    assert _bits(out._dev) == _bits(want) and out._dev.data_ptr() != ptr
    assert int(want.shape[0]) == (len(x) * 100) // int(rate)
    if copy:
        assert out is not dev and out.stats is not dev.stats
        assert dev._dev is before and dev._dev.data_ptr() == ptr and _bits(dev._dev) == x.tobytes() and dev._data is None
        assert dev.stats.npts == len(x) and dev.stats.sampling_rate == rate
    else:
        assert out is dev
    host_want = RS.resample_array(x, rate, 100.0)
    got = RS.resample_trace(host, 100.0, copy=copy, fourier_on_device=True)
    _on_host(got, host_want, 100.0)
    if copy:
        assert got is not host and host.data.tobytes() == x.tobytes() and host.stats.sampling_rate == rate
        assert host.stats.npts == len(x)
    else:
        assert got is host


def test_a_trace_already_at_the_rate_is_returned_as_it_is():
    dev, host, _ = _pair(100.0)
    before = dev._dev
    assert RS.resample_trace(dev, 100.0) is dev and dev._dev is before and RS.resample_trace(host, 100.0, copy=False) is host


# ------------------------------------------------------------------------------------------------------------- refusal
def _one_warning(record, text):
    assert [(str(w.message), w.category) for w in record] == [(text, UserWarning)]


def test_a_refused_filter_says_so_in_full_and_answers_from_the_host():
    dev, _, x = _pair(100.0)
    six = dict(freqmin=1, freqmax=20, corners=6)  # six sections: the kernel is built for four
    with pytest.raises(_lib.VolpickHipError, match="n_sections = 6") as e:
        SG.sos_filter_device(dev._dev, SG.butter_sos("bandpass", 100.0, **six))
    with pytest.warns(UserWarning) as record:
        assert dev.filter("bandpass", **six) is dev
    _one_warning(record, f"XX.T..HHZ: filtering on the device refused ({e.value}); filtering on the host")
    _on_host(dev, SG.filter_array(x, "bandpass", 100.0, **six), 100.0)


def test_a_refused_trigger_says_so_in_full_and_answers_from_the_host():
    import torch

    n = MAX_NLTA + 500
    dev, _, x = _pair(100.0, _samples(n, seed=8))
    lta = (MAX_NLTA + 1.5) / 100.0
    assert TR._windows(dev, 5.0, lta) == (500, MAX_NLTA + 1)
    with pytest.raises(_lib.VolpickHipError, match="65536") as e:
        TR.sta_lta_device(dev._dev, "recstalta", 500, MAX_NLTA + 1, torch.float32)
    with pytest.warns(UserWarning) as record:
        assert dev.trigger("recstalta", sta=5.0, lta=lta) is dev
    _one_warning(record, f"XX.T..HHZ: STA/LTA on the device refused ({e.value}); STA/LTA on the host")
    _on_host(dev, TR.recursive_sta_lta(x, 500, MAX_NLTA + 1), 100.0)


def test_a_float16_tensor_takes_the_host_path_without_a_warning():
    import torch

    x16 = (_samples(2000) / 8.0).astype(np.float16)
    steps = dict(_in_place_ops())
    steps["resample"] = (lambda tr: RS.resample_trace(tr, 50.0, copy=False, fourier_on_device=True), None,
                         lambda x: RS.resample_array(x, 100.0, 50.0))
    for name, (method, _, host_fn) in steps.items():
        tr = va.Trace(header=dict(HDR, sampling_rate=100.0), device_data=torch.from_numpy(x16).cuda())
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert method(tr) is tr, name
        _on_host(tr, host_fn(x16), 50.0 if name == "resample" else 100.0)


# -------------------------------------------------------------------------------------------------------------- upload
UPLOADED_AS = {np.int16: "torch.float32", np.int32: "torch.int32", np.float32: "torch.float32", np.float64: "torch.float64"}


@pytest.mark.parametrize("dtype", list(UPLOADED_AS), ids=lambda d: np.dtype(d).name)
def test_one_upload_rule_for_to_device_and_spectrogram(dtype, monkeypatch):
    import torch

    x = np.round(_samples(3000)).astype(dtype)
    host = va.Trace(x, dict(HDR, sampling_rate=100.0))
    dev = va.to_device(va.Stream([host]))[0]
    assert dev._data is None and dev._dev.is_cuda and str(dev._dev.dtype) == UPLOADED_AS[dtype]
    assert np.array_equal(dev._dev.cpu().numpy(), x) and dict(dev.stats) == dict(host.stats) and dev.stats is not host.stats
    seen = []
    real = SP.spectrogram
    monkeypatch.setattr(SP, "spectrogram", lambda t, *a, **kw: (seen.append(t), real(t, *a, **kw))[1])
    got = host.spectrogram()
    assert host._dev is None  # the upload is the call's own: the trace stays a host trace
    want = dev.spectrogram()
    assert len(seen) == 2 and seen[1] is dev._dev and dev._data is None  # a device trace is read where it lies
    assert seen[0].is_cuda and str(seen[0].dtype) == UPLOADED_AS[dtype] and torch.equal(seen[0], dev._dev)
    assert _bits(got.data) == _bits(want.data) and np.array_equal(got.freq, want.freq) and np.array_equal(got.time, want.time)


def test_each_masked_refusal_keeps_its_own_sentence():
    masked = va.Trace(np.ma.masked_array(_samples(1000), mask=np.arange(1000) % 97 == 0), dict(HDR, sampling_rate=100.0))
    for call, text in ((lambda: va.to_device(va.Stream([masked])),
                        "masked traces cannot be moved to the device; split the stream at its gaps first"),
                       (lambda: masked.spectrogram(),
                        "masked traces have no spectrogram; split the stream at its gaps first")):
        with pytest.raises(NotImplementedError, match="^" + re.escape(text) + "$"):
            call()


def test_a_trace_already_on_the_device_is_shared_not_copied():
    dev, host, _ = _pair(100.0)
    again = va.to_device(va.Stream([dev, host]))
    assert again[0] is not dev and again[0]._dev is dev._dev and again[0].stats is not dev.stats
    assert again[1]._dev.is_cuda and again[1]._dev.data_ptr() != dev._dev.data_ptr() and host._dev is None
