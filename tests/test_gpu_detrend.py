"""Device detrend (``vp_detrend``, volpick_amd/csrc/sosfilt.hip) against scipy and the closed forms, through the C ABI and
``detrend_device``: the three types x the three input kinds at n = 2, 3, one sample past a tile and 400 003, every sample within
``2^-22 max|x|`` (tests/sosfilt_f64.py: float64 sums, one rounding to float32 at the end); refusals at n = 1.

The least-squares line in closed form (index centred on (n - 1) / 2) differs from scipy's lstsq by float64 noise, under 1e-8 of
the bound; the test prints it."""
import ctypes as C

import numpy as np
import pytest

from tests import sosfilt_f64 as S
from volpick_amd import _lib
from volpick_amd.signal import DETREND_TYPES, detrend_array

pytestmark = pytest.mark.gpu

VP_ERR_INVALID = -1
LENGTHS = (2, 3, S.TILE + 1, 400_003)


def _call(dev_in, kind, n, type_code, dev_out):
    return _lib.load().vp_detrend(0, C.c_void_p(dev_in.data_ptr()), kind, n, type_code, C.c_void_p(dev_out.data_ptr()))


def _closed_form(x, type):
    n = len(x)
    if type == "simple":
        return x - (x[0] + np.arange(n) * (x[-1] - x[0]) / float(n - 1))
    if type in ("demean", "constant"):
        return x - x.sum() / n
    u = np.arange(n) - 0.5 * (n - 1)
    return x - (x.sum() / n + u * ((u * x).sum() / (n * (n * n - 1.0) / 12.0)))


@pytest.mark.parametrize("kind_name", list(S.KINDS))
@pytest.mark.parametrize("type", ("demean", "linear", "simple"))
def test_three_types_against_scipy_and_the_closed_form(type, kind_name):
    import torch

    kind, dtype = S.KINDS[kind_name]
    for n in LENGTHS:
        x = S.trace(n)
        want = detrend_array(x, type)
        closed = _closed_form(x, type)
        print(f"{type} n={n}: closed form vs scipy {S.ratio(closed, want, x):.2e} of the bound")
        assert S.ratio(closed, want, x) < 1e-6
        d = torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).cuda()
        out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_call(d, kind, n, DETREND_TYPES[type], out), "vp_detrend")
        got = out.cpu().numpy()
        r, rc = S.ratio(got, want, x), S.ratio(got, closed, x)
        print(f"{type} {kind_name} n={n}: worst |got - want| / bound = {r:.4f} (scipy), {rc:.4f} (closed form)")
        assert r <= 1.0 and rc <= 1.0
        if type == "simple":
            assert got[0] == 0.0 and got[-1] == 0.0


def test_refusals_and_the_python_surface():
    import torch

    from volpick_amd import VolpickHipError
    from volpick_amd.signal import detrend_device

    x = S.trace(5000)
    d = torch.from_numpy(x.astype(np.int32)).cuda()
    out = torch.full((5000,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    cases = (("linear, n = 1", lambda: _call(d, 0, 1, 1, out)), ("simple, n = 1", lambda: _call(d, 0, 1, 2, out)),
             ("type", lambda: _call(d, 0, 5000, 3, out)), ("in_kind", lambda: _call(d, 5, 5000, 0, out)),
             ("n < 0", lambda: _call(d, 0, -2, 0, out)), ("overlap", lambda: _call(d, 0, 5000, 0, d)))
    for what, call in cases:
        rc = call()
        msg = _lib.last_error()
        print(f"{what}: {rc} {msg}")
        assert rc == VP_ERR_INVALID and "vp_detrend" in msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert _call(d, 0, 1, 0, out) == 0 and float(out[0]) == 0.0 and float(out[1]) == -7.0  # the mean of one sample is itself
    with pytest.raises(VolpickHipError, match="two samples"):
        detrend_device(d[:1], "linear")
    with pytest.raises(ValueError):
        detrend_device(d, "polynomial")
    y = detrend_device(d, "constant")
    assert y.is_cuda and y.dtype == torch.float32 and S.ratio(y.cpu().numpy(), detrend_array(x, "demean"), x) <= 1.0
    twice = detrend_device(d, "linear")
    assert torch.equal(twice, detrend_device(d, "linear"))  # fixed summation order: the same bits
