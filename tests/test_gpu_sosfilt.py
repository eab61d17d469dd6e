"""Device filter (volpick_amd/csrc/sosfilt.hip) against the float64 host path (tests/sosfilt_f64.py; the bound's teeth:
tests/test_sosfilt_f64_cpu.py), through the C ABI (``vp_sos_filter``).

1. every filter of the set x input kind, one-pass and zero-phase, at every seam length, within ``2^-22 max|x|`` on every sample;
2. a trace of more tiles than the carry launch scans at a time through the 0.01 Hz high-pass; 3. two calls give the same bits;
4. a NaN mid-piece, at a piece seam, at a tile seam: one pass is right ahead of it and NaN from it on, zero-phase is NaN
everywhere, as scipy; 5. the refusals leave ``out`` untouched and the library usable; ``n == 0`` does nothing.

Every case prints its figure (worst |got - want| / bound) before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import sosfilt_f64 as S
from volpick_amd import _lib

pytestmark = pytest.mark.gpu

VP_ERR_INVALID = -1
SENTINEL = -7.0


def _call(dev_in, kind, n, sos, zerophase, dev_out, device=0):
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    return _lib.load().vp_sos_filter(device, C.c_void_p(dev_in.data_ptr()), kind, n, sos.ctypes.data_as(C.POINTER(C.c_double)),
                                     len(sos), int(zerophase), C.c_void_p(dev_out.data_ptr()))


def _filter(x, sos, zerophase, kind_name):
    """x (float64 array) as `kind_name` samples on the device -> float32 host array, through the C ABI."""
    import torch

    kind, dtype = S.KINDS[kind_name]
    d = torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).cuda()
    out = torch.full((len(x),), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_call(d, kind, len(x), sos, zerophase, out), "vp_sos_filter")
    return out.cpu().numpy()


@pytest.mark.parametrize("kind_name", list(S.KINDS))
@pytest.mark.parametrize("name", list(S.FILTERS))
def test_filter_set_and_input_kinds_within_the_bound_at_every_seam(name, kind_name):
    sos = S.sos_of(name)
    for zerophase in (False, True):
        for n in S.LENGTHS:
            x = S.trace(n)
            got = _filter(x, sos, zerophase, kind_name)
            r = S.ratio(got, S.want(name, n, zerophase), x)
            print(f"{name} {kind_name} zerophase={zerophase} n={n}: worst |got - want| / bound = {r:.4f}")
            assert got.dtype == np.float32
            assert r <= 1.0


@pytest.mark.parametrize("zerophase", (False, True))
def test_more_tiles_than_the_carry_scans_at_a_time(zerophase):
    name, n = "highpass 0.01 Hz", S.N_LONG
    assert -(-n // S.TILE) > S.CARRY_WIDTH  # 301 tiles against a scan of 256
    x = S.trace(n)
    got = _filter(x, S.sos_of(name), zerophase, "int32")
    want = S.want(name, n, zerophase)
    r = S.ratio(got, want, x)
    print(f"{name} zerophase={zerophase} n={n}: worst |got - want| / bound = {r:.4f}")
    assert r <= 1.0
    for sl in (slice(0, 2000), slice(S.CARRY_WIDTH * S.TILE - 1000, S.CARRY_WIDTH * S.TILE + 1000), slice(-2000, None)):
        assert S.ratio(got[sl], want[sl], x) <= 1.0


def test_two_calls_give_the_same_bits():
    x = S.trace(40_003)
    for name in ("highpass 0.3 Hz", "bandpass 1-20 Hz"):
        for zerophase in (False, True):
            a = _filter(x, S.sos_of(name), zerophase, "int32")
            b = _filter(x, S.sos_of(name), zerophase, "int32")
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("at", (S.TILE + 5 * S.PIECE + 17, S.TILE + 5 * S.PIECE, 2 * S.TILE), ids=("mid-piece", "piece seam", "tile seam"))
def test_nan_semantics_are_scipys(at):
    from volpick_amd.signal import filter_array

    n = 40_003
    x = S.trace(n).astype(np.float32)
    x[at] = np.nan
    for name in ("highpass 0.3 Hz", "bandpass 1-20 Hz", "highpass 1 Hz, 3 corners"):
        kind, opts = S.FILTERS[name]
        one = _filter(x.astype(np.float64), S.sos_of(name), False, "float32")
        want = filter_array(x, kind, S.DF, **opts)
        assert np.isfinite(want[:at]).all() and np.isnan(want[at:]).all()  # what scipy answers
        r = S.ratio(one[:at], want[:at], S.trace(n))
        print(f"{name}, NaN at {at}: ahead of it {r:.4f}")
        assert r <= 1.0
        assert np.isnan(one[at:]).all()
        both = _filter(x.astype(np.float64), S.sos_of(name), True, "float32")
        assert np.isnan(filter_array(x, kind, S.DF, zerophase=True, **opts)).all()
        assert np.isnan(both).all()
    clean = S.trace(n)  # nothing outlives the call
    assert S.ratio(_filter(clean, S.sos_of("highpass 0.3 Hz"), True, "float32"), S.want("highpass 0.3 Hz", n, True), clean) <= 1.0


def test_refusals_leave_out_untouched_and_the_library_usable():
    import torch

    n = 10_000
    x = S.trace(n)
    d = torch.from_numpy(x.astype(np.int32)).cuda()
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    sos = S.sos_of("highpass 0.3 Hz")
    kind = S.KINDS["int32"][0]
    unstable = sos.copy()
    unstable[0, 4:] = (-2.0, 1.0)  # a double pole AT 1
    outside = sos.copy()
    outside[1, 4:] = (0.0, 1.21)  # poles of radius 1.1
    torch.cuda.synchronize()
    cases = [
        ("5 sections", lambda: _call(d, kind, n, np.tile(sos, (3, 1))[:5], 0, out)),
        ("0 sections", lambda: _call(d, kind, n, sos[:0].reshape(0, 6), 0, out)),
        ("pole on the circle", lambda: _call(d, kind, n, unstable, 0, out)),
        ("pole outside", lambda: _call(d, kind, n, outside, 1, out)),
        ("a0", lambda: _call(d, kind, n, sos * 2.0, 0, out)),
        ("n < 0", lambda: _call(d, kind, -1, sos, 0, out)),
        ("in_kind", lambda: _call(d, 3, n, sos, 0, out)),
        ("overlap", lambda: _call(d, kind, n, sos, 0, d)),
    ]
    for what, call in cases:
        rc = call()
        msg = _lib.last_error()
        print(f"{what}: {rc} {msg}")
        assert rc == VP_ERR_INVALID and "vp_sos_filter" in msg
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    lib = _lib.load()
    null = lib.vp_sos_filter(0, None, kind, n, sos.ctypes.data_as(C.POINTER(C.c_double)), 2, 0, C.c_void_p(out.data_ptr()))
    assert null == VP_ERR_INVALID and bool((out == SENTINEL).all())
    assert _call(d, kind, 0, sos, 1, out) == 0 and bool((out == SENTINEL).all())  # n == 0: nothing to do
    assert bool((d.cpu() == torch.from_numpy(x.astype(np.int32))).all())
    got = _filter(x, sos, False, "int32")  # a call after the refusals still works
    assert S.ratio(got, S.want("highpass 0.3 Hz", n, False), x) <= 1.0


def test_python_surface_and_scratch_release():
    import torch

    from volpick_amd import VolpickHipError
    from volpick_amd.signal import release_filter_scratch, sos_filter_device

    n = 40_003
    x = S.trace(n)
    d = torch.from_numpy(x.astype(np.int32)).cuda()
    y = sos_filter_device(d, S.sos_of("bandpass 1-20 Hz"), zerophase=True)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == d.shape
    assert S.ratio(y.cpu().numpy(), S.want("bandpass 1-20 Hz", n, True), x) <= 1.0
    assert sos_filter_device(d[:0], S.sos_of("lowpass 20 Hz")).shape == (0,)
    with pytest.raises(VolpickHipError, match="n_sections"):
        sos_filter_device(d, np.tile(S.sos_of("bandpass 1-20 Hz"), (2, 1)))
    with pytest.raises(TypeError):
        sos_filter_device(d.cpu(), S.sos_of("lowpass 20 Hz"))
    freed = release_filter_scratch(0)
    assert freed >= 8 * n  # the float64 intermediate of the zero-phase call
    assert release_filter_scratch(0) == 0
    assert S.ratio(sos_filter_device(d, S.sos_of("lowpass 20 Hz")).cpu().numpy(), S.want("lowpass 20 Hz", n, False), x) <= 1.0
