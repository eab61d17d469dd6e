"""Device decimation (volpick_amd/csrc/resample.hip) against the float64 host path (tests/decimate_f64.py; the bound's teeth:
tests/test_decimate_f64_cpu.py), through the C ABI (``vp_decimate_lowpass``) and the public Python surface.

1. every factor x input kind at N = 400 003 within ``2^-22 max|x|`` on every output sample; 2. the edges: traces shorter than
any warm-up, lengths at the tile seams, the first and last 2 000 outputs of the long case on their own; 3. one component of a
200 Hz station-day; 4. a NaN / an Inf anywhere -> every output NaN; 5. argument errors; 6. a device-resident 200 Hz miniSEED
file stays on the device through ``_group_stream`` / ``classify``; 7. its picks against the host path's, both models, inside the
project's parity gate; 8. ``to_device`` of the host stream gives the device-resident read's picks bit for bit.

Every case prints its figure (worst |got - want| / bound, worst difference of a pick's peak value) before it asserts; LOG.md,
"Decimation on the device", says which of them have been measured on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from oracle import mseed as OM
from tests import mseed_util
from tests.decimate_f64 import FACTORS, KINDS, N_LONG, RATE_OUT, TILE, counts, ratio, want64
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd.resample import lowpass_sos
from volpick_amd.synthetic import synthetic_stream_array

pytestmark = pytest.mark.gpu

VP_ERR_INVALID, VP_ERR_UNSUPPORTED = -1, -4


def _call(dev_in, kind, n, sos, k, dev_out, out_len, device=0):
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    return _lib.load().vp_decimate_lowpass(device, C.c_void_p(dev_in.data_ptr()), kind, n,
                                           sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos), k,
                                           C.c_void_p(dev_out.data_ptr()), out_len)


def _decimate(x, k, kind_name):
    """x (float64 array of integers) as `kind_name` samples on the device -> float32 host array, through the C ABI."""
    import torch

    kind, dtype = KINDS[kind_name]
    d = torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).cuda()
    out = torch.full(((len(x) + k - 1) // k,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_call(d, kind, len(x), lowpass_sos(RATE_OUT * 0.5, RATE_OUT * k), k, out, out.shape[0]), "vp_decimate_lowpass")
    return out.cpu().numpy()


@pytest.mark.parametrize("kind_name", list(KINDS))
@pytest.mark.parametrize("k", FACTORS)
def test_every_factor_and_input_kind_within_the_bound(k, kind_name):
    x = counts(N_LONG, 100 + k)
    want = want64(x, k)
    got = _decimate(x, k, kind_name)
    r = ratio(got, want, x)
    print(f"decimate k={k} {kind_name}: worst |got - want| / bound = {r:.4f}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert r <= 1.0
    # the two ends on their own: an edge or seam error cannot hide in a maximum taken elsewhere
    for sl in (slice(0, 2000), slice(-2000, None)):
        r_edge = ratio(got[sl], want[sl], x)
        print(f"  outputs {sl.start}:{sl.stop}: {r_edge:.4f}")
        assert r_edge <= 1.0


@pytest.mark.parametrize("n", (1, 7, 50, TILE - 1, TILE, TILE + 1, 2 * TILE + 33))
def test_short_traces_and_tile_seams(n):
    for k in FACTORS:
        x = counts(n, 7 * n + k)
        for kind_name in ("int32", "float64"):
            got = _decimate(x, k, kind_name)
            r = ratio(got, want64(x, k), x)
            print(f"n={n} k={k} {kind_name}: {r:.4f}")
            assert r <= 1.0


def test_component_day_at_200_hz_and_scratch_release():
    from volpick_amd.resample import release_decimate_scratch

    n = 17_280_000
    x = counts(n, 2)
    got = _decimate(x, 2, "int32")
    r = ratio(got, want64(x, 2), x)
    print(f"component-day, k=2: worst |got - want| / bound = {r:.4f}")
    assert r <= 1.0
    freed = release_decimate_scratch(0)
    print(f"scratch released: {freed} bytes")
    assert freed >= 8 * n  # float64 intermediate, 8 bytes per input sample
    assert release_decimate_scratch(0) == 0
    small = counts(5000, 3)  # the next call allocates again
    assert ratio(_decimate(small, 2, "int32"), want64(small, 2), small) <= 1.0


@pytest.mark.parametrize("poison", (np.nan, np.inf))
@pytest.mark.parametrize("k", (2, 10))
def test_one_nonfinite_sample_makes_every_output_nan(poison, k):
    import torch

    x = counts(100_003, 5).astype(np.float32)
    x[50_000] = poison
    d = torch.from_numpy(x).cuda()
    out = torch.zeros((len(x) + k - 1) // k, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_call(d, KINDS["float32"][0], len(x), lowpass_sos(RATE_OUT * 0.5, RATE_OUT * k), k, out, out.shape[0]))
    assert np.isnan(out.cpu().numpy()).all()
    # what the whole-trace filter answers
    assert np.isnan(want64(x, k)).all()
    # the flag does not outlive the call
    clean = counts(100_003, 5)
    assert ratio(_decimate(clean, k, "float32"), want64(clean, k), clean) <= 1.0


def test_argument_errors_leave_the_library_usable():
    import torch

    x = counts(10_000, 9)
    d = torch.from_numpy(x.astype(np.int32)).cuda()
    out = torch.zeros(5000, dtype=torch.float32, device="cuda")
    sos2 = lowpass_sos(50.0, 200.0)
    kind = KINDS["int32"][0]
    torch.cuda.synchronize()
    cases = [
        ("factor", lambda: _call(d, kind, 10_000, sos2, 1, out, 5000), VP_ERR_INVALID),
        ("out_len", lambda: _call(d, kind, 10_000, sos2, 2, out, 4999), VP_ERR_INVALID),
        ("in_kind", lambda: _call(d, 3, 10_000, sos2, 2, out, 5000), VP_ERR_INVALID),
        ("n", lambda: _call(d, kind, 0, sos2, 2, out, 0), VP_ERR_INVALID),
        ("n_sections", lambda: _call(d, kind, 10_000, np.tile(sos2, (3, 1))[:5], 2, out, 5000), VP_ERR_INVALID),
        ("a0", lambda: _call(d, kind, 10_000, sos2 * 2.0, 2, out, 5000), VP_ERR_INVALID),
        # a pole radius of 0.995 needs a warm-up of ~5500 samples: beyond the tile
        ("warm-up", lambda: _call(d, kind, 10_000, lowpass_sos(50.0, 100.0 * 250), 250, out[:40], 40), VP_ERR_UNSUPPORTED),
    ]
    for what, call, code in cases:
        rc = call()
        msg = _lib.last_error()
        print(f"{what}: {rc} {msg}")
        assert rc == code and "vp_decimate_lowpass" in msg
    lib = _lib.load()
    null = lib.vp_decimate_lowpass(0, None, kind, 10_000, sos2.ctypes.data_as(C.POINTER(C.c_double)), 2, 2,
                                   C.c_void_p(out.data_ptr()), 5000)
    assert null == VP_ERR_INVALID
    assert ratio(_decimate(x, 2, "int32"), want64(x, 2), x) <= 1.0
    # factors up to 20 are supported, and 40 still fits
    for k in (20, 40):
        xs = counts(50_001, k)
        assert ratio(_decimate(xs, k, "int32"), want64(xs, k), xs) <= 1.0


# ------------------------------------------------------------------------------------------ stream handling
def _file_200hz():
    """A 200 Hz three-component miniSEED file: the 100 Hz synthetic stream of tests/test_gpu_phasenet.py taken to 200 Hz with the
    Fourier method, scaled to counts."""
    from volpick_amd.resample import resample_fourier

    data, _, _ = synthetic_stream_array(60_000, seed=1001, n_events=6)
    fast = np.stack([resample_fourier(data[i].astype(np.float64), 100.0, 200.0, window=None) for i in range(3)])
    cnt = np.round(fast * (1.0e5 / np.abs(fast).max())).astype(np.int32)
    traces = mseed_util.three_component(10, np.random.default_rng(0), rate=200.0)
    for tr, row in zip(traces, cnt):
        tr["data"] = row
    return mseed_util.file_bytes(traces, reclen=4096, encoding=OM.ENC_INT32)  # (plain int32: Steim-packing 360 000 samples in Python takes 45 s)


@pytest.fixture(scope="module")
def buf200():
    return _file_200hz()


def test_device_resident_200hz_stream_stays_on_the_device(buf200):
    import torch

    import volpick_amd as va
    from volpick_amd.models import _group_stream

    st = va.read(buf200, device_resident=True)
    assert len(st) == 3 and all(tr.stats.sampling_rate == 200.0 and tr._dev is not None and tr._data is None for tr in st)
    before = [tr._dev for tr in st]
    groups = list(_group_stream(st, "ZNE", 100.0, True, 3001))
    assert len(groups) == 1
    block = groups[0]["data"]
    assert torch.is_tensor(block) and block.is_cuda and block.dtype == torch.float32 and tuple(block.shape) == (3, 60_000)
    # the block is the host path's answer within the bound
    host = va.read(buf200)
    order = {tr.stats.channel[-1]: tr for tr in host}
    for c, comp in enumerate("ZNE"):
        x = order[comp].data.astype(np.float64)
        assert ratio(block[c].cpu().numpy(), want64(x, 2), x) <= 1.0
    model = PhaseNet.from_pretrained("volpick").cuda()
    picks = model.classify(st).picks
    assert len(picks) >= 6
    for tr, d in zip(st, before):  # copy=True: the caller's traces are untouched and were never copied to the host
        assert tr.stats.sampling_rate == 200.0 and tr.stats.npts == 120_000 and tr._dev is d and tr._data is None
    picks_inplace = model.classify(st, copy=False).picks
    for tr in st:  # copy=False: resampled in place, as upstream does -- still on the device
        assert tr.stats.sampling_rate == 100.0 and tr.stats.npts == 60_000 and len(tr) == 60_000
        assert tr._dev is not None and tr._dev.is_cuda and tr._dev.shape[0] == 60_000 and tr._data is None
    assert _pick_rows(picks_inplace) == _pick_rows(picks)


def _pick_rows(picks):
    return sorted((p.trace_id, p.phase, p.peak_time.timestamp, float(p.peak_value)) for p in picks)


@pytest.mark.parametrize("cls", (PhaseNet, EQTransformer))
def test_picks_match_the_host_path_and_to_device_matches_the_resident_read(cls, buf200):
    import volpick_amd as va

    model = cls.from_pretrained("volpick").cuda()
    ref = _pick_rows(model.classify(va.read(buf200)).picks)  # host traces, host scipy path
    got = _pick_rows(model.classify(va.read(buf200, device_resident=True)).picks)
    assert len(ref) >= 6 and len(got) == len(ref)
    worst = 0.0
    for a, b in zip(ref, got):
        assert a[0] == b[0] and a[1] == b[1]
        assert abs(a[2] - b[2]) <= 0.01
        worst = max(worst, abs(a[3] - b[3]))
    print(f"{cls.__name__}: {len(ref)} picks, worst |delta peak_value| device vs host resampling = {worst:.3e}")
    assert worst < 1e-4
    # to_device of the host stream: same samples, same path -> the same picks bit for bit
    host = va.read(buf200)
    moved = va.to_device(host)
    assert all(tr._dev is not None and tr._dev.is_cuda and tr._data is None for tr in moved)
    assert [str(tr._dev.dtype) for tr in moved] == ["torch.int32"] * 3
    assert all(a.stats.sampling_rate == 200.0 and a.id == b.id and a.stats.starttime == b.stats.starttime
               for a, b in zip(moved, host))
    assert _pick_rows(model.classify(moved).picks) == got


def test_to_device_keeps_dtypes_and_other_ratios_take_the_host_path():
    import volpick_amd as va
    from volpick_amd.resample import resample_array, resample_trace

    rng = np.random.default_rng(4)
    t0 = va.UTCDateTime("2021-03-04T05:06:07")
    st = va.Stream([va.Trace(rng.standard_normal(5000).astype(dt), dict(network="XX", station="A", channel="HHZ", starttime=t0,
                                                                       sampling_rate=250.0)) for dt in (np.float32, np.float64)])
    moved = va.to_device(st)
    assert [str(tr._dev.dtype) for tr in moved] == ["torch.float32", "torch.float64"]
    for tr, src in zip(moved, st):  # 250 -> 100 Hz: the Fourier method on the host, device-backed or not
        out = resample_trace(tr, 100.0)
        assert out is not tr and out._dev is None and out.stats.sampling_rate == 100.0
        assert np.array_equal(out.data, resample_array(src.data, 250.0, 100.0))
    # float64 device samples at an integer ratio go through the kernel as float64
    x = counts(30_000, 8)
    tr = va.to_device(va.Stream([va.Trace(x, dict(sampling_rate=500.0, channel="HHZ"))]))[0]
    out = resample_trace(tr, 100.0)
    assert out._dev is not None and out._data is None and out.stats.npts == 6000 and tr.stats.npts == 30_000
    assert ratio(out._dev.cpu().numpy(), want64(x, 5), x) <= 1.0
