"""Device Fourier resampling (volpick_amd/csrc/fourier.hip) against the float64 host path (tests/fourier_f64.py; the bound's
teeth: tests/test_fourier_f64_cpu.py), through the C ABI (``vp_resample_fourier``) and the public Python surface.

1. every rate x input kind at N = 400 003 within ``2^-22 max|x|`` on every output sample, the first and last 2 000 outputs on
their own; 2. the four parities of (N, num) and exact 2x zero-padding; 3. short traces, and for each pass count of the FFT the
two lengths on either side of the switch, for the forward and for the inverse transform; 4. a 50 Hz component-day (the largest
pass count) and the scratch release; 5. a NaN / an Inf anywhere -> every output NaN, and the flag does not outlive the call;
6. argument errors; 7. a device-resident 250 Hz miniSEED file stays on the device through ``_group_stream`` / ``classify``;
8. its picks against the host path's, both models, inside the project's parity gate, and ``to_device`` of the host stream
gives the device-resident read's picks bit for bit.

Every case prints its figure (worst |got - want| / bound, worst difference of a pick's peak value) before it asserts; LOG.md,
"Fourier resampling on the device", says which of them have been measured on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import mseed as OM
from tests import mseed_util
from tests.fourier_f64 import (KINDS, N_LONG, PASS_LIMITS, RATE_OUT, RATES, counts, fft_passes, fft_size, host_args,
                               length_for_passes, ratio, want64)
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd.synthetic import synthetic_stream_array

pytestmark = pytest.mark.gpu

VP_ERR_INVALID = -1


def _call(dev_in, kind, n, rate, num, df, dlf, dev_out, out_len, device=0):
    return _lib.load().vp_resample_fourier(device, C.c_void_p(dev_in.data_ptr()), kind, n, float(rate), RATE_OUT, num, df, dlf,
                                           C.c_void_p(dev_out.data_ptr()), out_len)


def _resample(x, rate, kind_name):
    """x (float64 array) as `kind_name` samples on the device -> float32 host array, through the C ABI."""
    import torch

    kind, dtype = KINDS[kind_name]
    num, df, dlf = host_args(len(x), float(rate))
    d = torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).cuda()
    out = torch.full((num,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_call(d, kind, len(x), rate, num, df, dlf, out, num), "vp_resample_fourier")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _long_case(rate):
    x = counts(N_LONG, 100 + rate)
    want = want64(x, rate)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("kind_name", list(KINDS))
@pytest.mark.parametrize("rate", RATES)
def test_every_rate_and_input_kind_within_the_bound(rate, kind_name):
    x, want = _long_case(rate)
    got = _resample(x, rate, kind_name)
    r = ratio(got, want, x)
    print(f"fourier {rate} -> 100 Hz {kind_name}: worst |got - want| / bound = {r:.4f}")
    assert got.dtype == np.float32 and got.shape == want.shape == (host_args(N_LONG, float(rate))[0],)
    assert r <= 1.0
    # the two ends on their own: an edge error cannot hide in a maximum taken elsewhere
    for sl in (slice(0, 2000), slice(-2000, None)):
        r_edge = ratio(got[sl], want[sl], x)
        print(f"  outputs {sl.start}:{sl.stop}: {r_edge:.4f}")
        assert r_edge <= 1.0


@pytest.mark.parametrize("n,rate,n_odd,num_odd", ((5000, 250, 0, 0), (5001, 250, 1, 0), (4999, 125, 1, 1), (5004, 125, 0, 1),
                                                  (5000, 50, 0, 0)))
def test_parities_of_input_and_output_length(n, rate, n_odd, num_odd):
    num = host_args(n, float(rate))[0]
    assert n % 2 == n_odd and num % 2 == num_odd
    if rate == 50:
        assert num == 2 * n  # exact 2x zero-padding of the spectrum
    x = counts(n, 11 * n + rate)
    for kind_name in ("int32", "float64"):
        r = ratio(_resample(x, rate, kind_name), want64(x, rate), x)
        print(f"n={n} ({rate} Hz) -> num={num} {kind_name}: {r:.4f}")
        assert r <= 1.0


@pytest.mark.parametrize("n", (1, 2, 3, 7, 50))
def test_short_traces(n):
    ran = 0
    for rate in RATES:
        if host_args(n, float(rate))[0] < 1:  # N = 1 gives an output sample at the upsampling rates only
            continue
        x = counts(n, 7 * n + rate)
        for kind_name in ("int32", "float64"):
            r = ratio(_resample(x, rate, kind_name), want64(x, rate), x)
            print(f"n={n} {rate} Hz {kind_name}: {r:.4f}")
            assert r <= 1.0
            ran += 1
    assert ran >= 6


def _n_for_num(num):
    """(n, rate) whose output length is `num`, an upsampling rate first so that the inverse transform is the larger one."""
    for rate in sorted(RATES):
        f = rate / RATE_OUT
        for n in range(max(1, int(num * f) - 2), int(num * f) + 4):
            if host_args(n, float(rate))[0] == num:
                return n, rate
    raise AssertionError(f"no rate gives {num} output samples")


@pytest.mark.parametrize("side", (0, 1))
@pytest.mark.parametrize("npass", (1, 2))
@pytest.mark.parametrize("which", ("forward", "inverse"))
def test_lengths_on_either_side_of_a_pass_count_switch(which, npass, side):
    length = length_for_passes(npass, side)
    assert len(fft_passes(fft_size(length))) == npass + side and (1 << fft_size(length)) == PASS_LIMITS[npass - 1] << side
    n, rate = (length, 250) if which == "forward" else _n_for_num(length)
    num = host_args(n, float(rate))[0]
    assert (n if which == "forward" else num) == length
    x = counts(n, 3 * n + rate)
    r = ratio(_resample(x, rate, "int32"), want64(x, rate), x)
    print(f"{which} transform of {length} points ({npass + side} pass(es)), n={n} at {rate} Hz -> {num}: {r:.4f}")
    assert r <= 1.0


def test_component_day_at_50_hz_and_scratch_release():
    from volpick_amd.resample import release_fourier_scratch

    n = 4_320_000
    assert len(fft_passes(fft_size(2 * n))) == 3 and fft_size(2 * n) == 25  # the largest pass count
    x = counts(n, 2)
    got = _resample(x, 50, "int32")
    assert got.shape == (8_640_000,)
    r = ratio(got, want64(x, 50), x)
    print(f"component-day, 50 -> 100 Hz: worst |got - want| / bound = {r:.4f}")
    assert r <= 1.0
    freed = release_fourier_scratch(0)
    print(f"scratch released: {freed} bytes")
    assert freed > 0
    assert release_fourier_scratch(0) == 0
    small = counts(5000, 3)  # the next call allocates again
    assert ratio(_resample(small, 250, "int32"), want64(small, 250), small) <= 1.0


@pytest.mark.parametrize("poison", (np.nan, np.inf))
@pytest.mark.parametrize("rate", (250, 40))
def test_one_nonfinite_sample_makes_every_output_nan(poison, rate):
    import torch

    x = counts(100_003, 5).astype(np.float32)
    x[50_000] = poison
    num, df, dlf = host_args(len(x), float(rate))
    d = torch.from_numpy(x).cuda()
    out = torch.zeros(num, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_call(d, KINDS["float32"][0], len(x), rate, num, df, dlf, out, num))
    assert np.isnan(out.cpu().numpy()).all()
    # what the host transform answers
    assert np.isnan(want64(x, rate)).all()
    # the flag does not outlive the call
    clean = counts(100_003, 5)
    r = ratio(_resample(clean, rate, "float32"), want64(clean, rate), clean)
    print(f"clean call after the poisoned one, {rate} Hz: {r:.4f}")
    assert r <= 1.0


def test_argument_errors_leave_the_library_usable():
    import torch

    from volpick_amd.resample import fourier_device

    x = counts(10_000, 9)
    d = torch.from_numpy(x.astype(np.int32)).cuda()
    out = torch.zeros(4000, dtype=torch.float32, device="cuda")
    kind = KINDS["int32"][0]
    num, df, dlf = host_args(10_000, 250.0)
    assert num == 4000
    torch.cuda.synchronize()
    cases = [
        ("num 0", lambda: _call(d, kind, 1, 250, 0, 250.0, float("nan"), out, 0)),  # N = 1 at 250 Hz: int(1 / 2.5) = 0
        ("out_len", lambda: _call(d, kind, 10_000, 250, num, df, dlf, out, 3999)),
        ("in_kind", lambda: _call(d, 3, 10_000, 250, num, df, dlf, out, num)),
        ("n", lambda: _call(d, kind, 0, 250, num, df, dlf, out, num)),
    ]
    for what, call in cases:
        rc = call()
        msg = _lib.last_error()
        print(f"{what}: {rc} {msg}")
        assert rc == VP_ERR_INVALID and "vp_resample_fourier" in msg
    lib = _lib.load()
    for null_in in (True, False):
        rc = lib.vp_resample_fourier(0, None if null_in else C.c_void_p(d.data_ptr()), kind, 10_000, 250.0, RATE_OUT, num, df,
                                     dlf, C.c_void_p(out.data_ptr()) if null_in else None, num)
        assert rc == VP_ERR_INVALID and "vp_resample_fourier" in _lib.last_error()
    assert ratio(_resample(x, 250, "int32"), want64(x, 250), x) <= 1.0
    for rate_in in (200.0, 100.0):  # the other branch, and nothing to do
        with pytest.raises(ValueError):
            fourier_device(d, rate_in, 100.0)
    with pytest.raises(ValueError):
        fourier_device(d[:1], 250.0, 100.0)  # no output sample
    y = fourier_device(d, 250.0, 100.0)
    assert y.is_cuda and y.dtype == torch.float32 and ratio(y.cpu().numpy(), want64(x, 250), x) <= 1.0


# ------------------------------------------------------------------------------------------ stream handling
def _file_250hz():
    """A 250 Hz three-component miniSEED file: the 100 Hz synthetic stream of tests/test_gpu_phasenet.py taken to 250 Hz with the
    Fourier method, scaled to counts (built the way tests/test_gpu_decimate.py builds its 200 Hz file)."""
    from volpick_amd.resample import resample_fourier

    data, _, _ = synthetic_stream_array(60_000, seed=1001, n_events=6)
    fast = np.stack([resample_fourier(data[i].astype(np.float64), 100.0, 250.0, window=None) for i in range(3)])
    assert fast.shape == (3, 150_000)
    cnt = np.round(fast * (1.0e5 / np.abs(fast).max())).astype(np.int32)
    traces = mseed_util.three_component(10, np.random.default_rng(0), rate=250.0)
    for tr, row in zip(traces, cnt):
        tr["data"] = row
    return mseed_util.file_bytes(traces, reclen=4096, encoding=OM.ENC_INT32)


@pytest.fixture(scope="module")
def buf250():
    return _file_250hz()


def test_device_resident_250hz_stream_stays_on_the_device(buf250):
    import torch

    import volpick_amd as va
    from volpick_amd.models import _group_stream
    from volpick_amd.resample import resample_trace

    st = va.read(buf250, device_resident=True)
    assert len(st) == 3 and all(tr.stats.sampling_rate == 250.0 and tr._dev is not None and tr._data is None for tr in st)
    before = [tr._dev for tr in st]
    groups = list(_group_stream(st, "ZNE", 100.0, True, 3001))
    assert len(groups) == 1
    block = groups[0]["data"]
    assert torch.is_tensor(block) and block.is_cuda and block.dtype == torch.float32 and tuple(block.shape) == (3, 60_000)
    # the block is the host path's answer within the bound
    host = va.read(buf250)
    order = {tr.stats.channel[-1]: tr for tr in host}
    for c, comp in enumerate("ZNE"):
        x = order[comp].data.astype(np.float64)
        r = ratio(block[c].cpu().numpy(), want64(x, 250), x)
        print(f"component {comp}: worst |block - host| / bound = {r:.4f}")
        assert r <= 1.0
    model = PhaseNet.from_pretrained("volpick").cuda()
    picks = model.classify(st).picks
    assert len(picks) >= 6
    for tr, d in zip(st, before):  # copy=True: the caller's traces are untouched and were never copied to the host
        assert tr.stats.sampling_rate == 250.0 and tr.stats.npts == 150_000 and tr._dev is d and tr._data is None
    # the default of resample_trace is still the host path
    out = resample_trace(st[0], 100.0)
    assert out is not st[0] and out._dev is None and out.stats.sampling_rate == 100.0 and len(out.data) == 60_000
    assert st[0]._dev is before[0] and st[0].stats.sampling_rate == 250.0
    picks_inplace = model.classify(st, copy=False).picks
    for tr in st:  # copy=False: resampled in place, as upstream does -- still on the device
        assert tr.stats.sampling_rate == 100.0 and tr.stats.npts == 60_000 and len(tr) == 60_000
        assert tr._dev is not None and tr._dev.is_cuda and tr._dev.shape[0] == 60_000 and tr._data is None
    assert _pick_rows(picks_inplace) == _pick_rows(picks)


def _pick_rows(picks):
    return sorted((p.trace_id, p.phase, p.peak_time.timestamp, float(p.peak_value)) for p in picks)


@pytest.mark.parametrize("cls", (PhaseNet, EQTransformer))
def test_picks_match_the_host_path_and_to_device_matches_the_resident_read(cls, buf250):
    import volpick_amd as va

    model = cls.from_pretrained("volpick").cuda()
    ref = _pick_rows(model.classify(va.read(buf250)).picks)  # host traces, host scipy path
    got = _pick_rows(model.classify(va.read(buf250, device_resident=True)).picks)
    assert len(ref) >= 6 and len(got) == len(ref)
    worst = 0.0
    for a, b in zip(ref, got):
        assert a[0] == b[0] and a[1] == b[1]
        assert abs(a[2] - b[2]) <= 0.01
        worst = max(worst, abs(a[3] - b[3]))
    print(f"{cls.__name__}: {len(ref)} picks, worst |delta peak_value| device vs host resampling = {worst:.3e}")
    assert worst < 1e-4
    # to_device of the host stream: same samples, same path -> the same picks bit for bit
    host = va.read(buf250)
    moved = va.to_device(host)
    assert all(tr._dev is not None and tr._dev.is_cuda and tr._data is None for tr in moved)
    assert [str(tr._dev.dtype) for tr in moved] == ["torch.int32"] * 3
    assert _pick_rows(model.classify(moved).picks) == got
