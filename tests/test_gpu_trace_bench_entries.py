"""The four timing entry points of the trace operations (``vp_sos_filter_bench``, ``vp_decimate_lowpass_bench``,
``vp_resample_fourier_bench``, ``vp_mseed_decode_bench``), which the tools and bench.py call and no other test does: each
returns VP_OK with finite positive times, leaves in ``out`` the bits the plain entry point writes for the same input, refuses
``iters`` = 0 with VP_ERR_INVALID and works on the next valid call.  What the plain entry points compute is the business of
test_gpu_sosfilt.py, test_gpu_decimate.py, test_gpu_fourier.py and test_gpu_mseed.py."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from volpick_amd import _lib
from volpick_amd.resample import fourier_args, lowpass_sos
from volpick_amd.signal import butter_sos

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
VP_OK, VP_ERR_INVALID = 0, -1
ITERS = 2
N = 3 * 8192 + 5  # four tiles of 8192 samples: the filter's carry launch runs
DP = C.POINTER(C.c_double)


def _sos(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(DP), len(a)


@pytest.fixture(scope="module")
def counts():
    import torch

    rng = np.random.default_rng(33)
    x = np.round(800.0 * rng.standard_normal(N) + 30000.0 * np.sin(np.arange(N) / 500.0) + 123456.0).astype(np.int32)
    return torch.from_numpy(x).cuda()


def _fresh(n, dtype=None):
    import torch

    out = torch.full((n,), -7, dtype=dtype or torch.float32, device="cuda")
    torch.cuda.synchronize()  # the library works on streams of its own
    return out


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_times(*times):
    for t in times:
        print(f"  {t.value:.6f} ms")
        assert math.isfinite(t.value) and t.value > 0.0


def _bench_then_refusal_then_bench(bench, out, want):
    """bench(iters, out) -> (rc, times): a valid call, iters = 0, a valid call again."""
    import torch

    for round_ in range(2):
        out.fill_(-7)
        torch.cuda.synchronize()
        rc, times = bench(ITERS, out)
        assert rc == VP_OK, _lib.last_error()
        _check_times(*times)
        assert _same_bits(out, want)
        if round_ == 0:
            rc, _ = bench(0, out)
            assert rc == VP_ERR_INVALID and "bad argument" in _lib.last_error()
            assert _same_bits(out, want)  # a refused call launches nothing


@pytest.mark.parametrize("zerophase", (0, 1))
def test_sos_filter_bench(counts, zerophase):
    lib = _lib.load()
    keep, sos, ns = _sos(butter_sos("bandpass", 100.0, freqmin=1.0, freqmax=20.0))
    want = _fresh(N)
    _lib.check(lib.vp_sos_filter(0, counts.data_ptr(), _lib.VP_SAMPLES_INT32, N, sos, ns, zerophase, want.data_ptr()), "vp_sos_filter")
    assert not (want == -7).all()

    def bench(iters, out):
        ms, ms_carry = C.c_float(-1), C.c_float(-1)
        rc = lib.vp_sos_filter_bench(0, counts.data_ptr(), _lib.VP_SAMPLES_INT32, N, sos, ns, zerophase, out.data_ptr(), iters,
                                     C.byref(ms), C.byref(ms_carry))
        return rc, (ms, ms_carry)

    _bench_then_refusal_then_bench(bench, _fresh(N), want)


def test_decimate_lowpass_bench(counts):
    lib = _lib.load()
    k = 2
    keep, sos, ns = _sos(lowpass_sos(50.0, 200.0))
    m = (N + k - 1) // k
    want = _fresh(m)
    _lib.check(lib.vp_decimate_lowpass(0, counts.data_ptr(), _lib.VP_SAMPLES_INT32, N, sos, ns, k, want.data_ptr(), m),
               "vp_decimate_lowpass")
    assert not (want == -7).all()

    def bench(iters, out):
        ms, ms_forward = C.c_float(-1), C.c_float(-1)
        rc = lib.vp_decimate_lowpass_bench(0, counts.data_ptr(), _lib.VP_SAMPLES_INT32, N, sos, ns, k, out.data_ptr(), m, iters,
                                           C.byref(ms), C.byref(ms_forward))
        return rc, (ms, ms_forward)

    _bench_then_refusal_then_bench(bench, _fresh(m), want)


def test_resample_fourier_bench(counts):
    lib = _lib.load()
    n, rate_in, rate_out = 5000, 250.0, 100.0
    num, df, d_large_f = fourier_args(n, rate_in, rate_out)
    assert num == 2000
    x = counts[:n].contiguous()
    want = _fresh(num)
    _lib.check(lib.vp_resample_fourier(0, x.data_ptr(), _lib.VP_SAMPLES_INT32, n, rate_in, rate_out, num, df, d_large_f,
                                       want.data_ptr(), num), "vp_resample_fourier")
    assert not (want == -7).all()

    def bench(iters, out):
        ms, ms_forward = C.c_float(-1), C.c_float(-1)
        rc = lib.vp_resample_fourier_bench(0, x.data_ptr(), _lib.VP_SAMPLES_INT32, n, rate_in, rate_out, num, df, d_large_f,
                                           out.data_ptr(), num, iters, C.byref(ms), C.byref(ms_forward))
        return rc, (ms, ms_forward)

    _bench_then_refusal_then_bench(bench, _fresh(num), want)


def test_mseed_decode_bench():
    import torch

    import volpick_amd.io as vio

    lib = _lib.load()
    buf = (ROOT / "tests" / "golden" / "bench_steim2_6min.mseed").read_bytes()
    recs = vio.scan_mseed(buf)
    ns = recs["nsamples"].astype(np.int64)
    index = np.ascontiguousarray(np.cumsum(ns) - ns, dtype=np.int64)
    index_p = index.ctypes.data_as(C.POINTER(C.c_int64))
    total = int(ns.sum())
    assert len(recs) == 36 and total > 0
    recs_c = (_lib.VpMseedRecord * len(recs)).from_buffer_copy(np.ascontiguousarray(recs).tobytes())
    dbuf = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    want = _fresh(total, torch.int32)
    torch.cuda.synchronize()
    _lib.check(lib.vp_mseed_decode(0, dbuf.data_ptr(), _lib.VP_MEM_DEVICE, len(buf), recs_c, index_p, None, len(recs),
                                   _lib.VP_SAMPLES_INT32, want.data_ptr(), _lib.VP_MEM_DEVICE, total, 0, None), "vp_mseed_decode")
    assert not (want == -7).all()

    def bench(iters, out):
        ms = C.c_float(-1)
        rc = lib.vp_mseed_decode_bench(0, dbuf.data_ptr(), len(buf), recs_c, index_p, len(recs), _lib.VP_SAMPLES_INT32,
                                       out.data_ptr(), total, iters, C.byref(ms))
        return rc, (ms,)

    _bench_then_refusal_then_bench(bench, _fresh(total, torch.int32), want)
