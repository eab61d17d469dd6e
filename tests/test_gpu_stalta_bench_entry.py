"""The timing entry point of the device STA/LTA (``vp_sta_lta_bench``), which tools/stalta_timing.py calls and no other test
does: VP_OK with a finite positive time, ``out`` bit-equal to what the plain entry point writes for the same input, ``iters``
= 0 refused with VP_ERR_INVALID, and the next valid call works.  What ``vp_sta_lta`` computes is the business of
tests/test_gpu_stalta.py."""
import ctypes as C
import math

import numpy as np
import pytest

from volpick_amd import _lib

pytestmark = pytest.mark.gpu

VP_OK, VP_ERR_INVALID = 0, -1
ITERS = 2
N = 3 * 8192 + 5  # four tiles of 8192 samples: the carry launches run
STRIDE = N + 11


@pytest.mark.parametrize("type_", (_lib.VP_STALTA_CLASSIC, _lib.VP_STALTA_RECURSIVE))
@pytest.mark.parametrize("out_kind", (_lib.VP_SAMPLES_FLOAT32, _lib.VP_SAMPLES_FLOAT64))
def test_sta_lta_bench(type_, out_kind):
    import torch

    lib = _lib.load()
    rng = np.random.default_rng(33)
    x = np.round(800.0 * rng.standard_normal((3, STRIDE)) + 123456.0).astype(np.int32)
    d = torch.from_numpy(x).cuda()
    dtype = torch.float32 if out_kind == _lib.VP_SAMPLES_FLOAT32 else torch.float64
    bits = torch.int32 if out_kind == _lib.VP_SAMPLES_FLOAT32 else torch.int64

    def fresh():
        out = torch.full((3, STRIDE), -7, dtype=dtype, device="cuda")
        torch.cuda.synchronize()  # the library works on streams of its own
        return out

    args = (0, C.c_void_p(d.data_ptr()), _lib.VP_SAMPLES_INT32, 3, STRIDE, N, type_, 50, 1000)
    want = fresh()
    _lib.check(lib.vp_sta_lta(*args, C.c_void_p(want.data_ptr()), out_kind), "vp_sta_lta")
    assert not (want[:, :N] == -7).any() and (want[:, N:] == -7).all()
    out = fresh()
    for round_ in range(2):
        out.fill_(-7)
        torch.cuda.synchronize()
        ms = C.c_float(-1)
        rc = lib.vp_sta_lta_bench(*args, C.c_void_p(out.data_ptr()), out_kind, ITERS, C.byref(ms))
        assert rc == VP_OK, _lib.last_error()
        print(f"  {ms.value:.6f} ms")
        assert math.isfinite(ms.value) and ms.value > 0.0
        assert torch.equal(out.view(bits), want.view(bits))
        if round_ == 0:
            rc = lib.vp_sta_lta_bench(*args, C.c_void_p(out.data_ptr()), out_kind, 0, C.byref(ms))
            assert rc == VP_ERR_INVALID and "bad argument" in _lib.last_error()
            assert torch.equal(out.view(bits), want.view(bits))  # a refused call launches nothing
