"""The device STA/LTA (``vp_sta_lta``) and the handle-free trigger scan (``vp_trigger_onset``) on an MI355X, through the C ABI and
through volpick_amd/trigger.py, against the extended-precision truth and the bars of tests/stalta_f64.py (whose teeth
tests/test_stalta_f64_cpu.py shows).  Nothing here was tuned on the kernel's output.

The one trace of more tiles than the carry launch scans at a time (recursive type) is checked against the float64 ``lfilter``
restatement at the sum of both bounds, twice the recursive bar: its extended-precision loop would take most of a minute."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import volpick_amd as va
from tests import stalta_f64 as S
from tests import trigger_cases as TC
from volpick_amd import _lib, trigger as TR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
VP_OK, VP_ERR_INVALID, VP_ERR_UNSUPPORTED = 0, -1, -4
TYPE = {"classic": _lib.VP_STALTA_CLASSIC, "recursive": _lib.VP_STALTA_RECURSIVE}
NAME = {"classic": "classicstalta", "recursive": "recstalta"}
T, P = S.T, S.P
N = 40_003
SMALL = ((5, 20), (50, 1000), (500, 2000))
I64 = C.POINTER(C.c_int64)


def _cuda(x, dtype=np.float64):
    import torch

    return torch.from_numpy(np.array(x, dtype=dtype)).cuda()  # (a copy: the helper's inputs are read-only)


def _run(kind, x, nsta, nlta, in_dtype=np.float64, out32=False):
    import torch

    y = TR.sta_lta_device(_cuda(x, in_dtype), NAME[kind], nsta, nlta, torch.float32 if out32 else None)
    assert y.dtype == (torch.float32 if out32 else torch.float64)
    return y.cpu().numpy()


def _check(kind, name, n, nsta, nlta, in_dtype=np.float64, out32=False, lead=0):
    x = S.zeros_then_noise(n, lead) if name == "zeros_then_noise" else S.ALL_INPUTS[name](n)
    got = _run(kind, x, nsta, nlta, in_dtype, out32)
    t = S.truth(kind, name, n, nsta, nlta, lead)
    r = S.ratio(kind, got, t, nsta, nlta, out32)
    print(f"{kind} {name} n={n} {nsta}/{nlta} {np.dtype(in_dtype).name}->{'f32' if out32 else 'f64'}: {r:.4f} of the bar")
    head = nlta if kind == "recursive" else nlta - 1
    assert not got[:head].any()  # the zeroed head, exactly
    assert r <= 1.0
    return got


@pytest.mark.parametrize("kind", list(TYPE))
@pytest.mark.parametrize("out32", (False, True))
@pytest.mark.parametrize("in_kind", list(S.KINDS))
def test_every_input_and_output_kind(kind, out32, in_kind):
    _check(kind, "plain", 2 * T + 5, 5, 20, S.KINDS[in_kind][1], out32)


@pytest.mark.parametrize("nsta,nlta", S.WINDOWS)
def test_seam_lengths(nsta, nlta):
    for n in S.seam_lengths(nlta):
        for kind in TYPE:
            _check(kind, "plain", n, nsta, nlta)


def test_more_tiles_than_the_carry_launch_scans_at_a_time():
    n, nsta, nlta = S.N_LONG, 500, 2000
    assert -(-n // T) > S.CARRY_WIDTH + 1
    x = S.counts(n, 5)
    got = _run("recursive", x, nsta, nlta)
    want = TR.recursive_sta_lta(x, nsta, nlta)
    bound = 2 * (6 * (np.arange(n) + 1.0) + 10) * S.U * np.abs(want)  # the kernel's bar plus the restatement's own
    worst = float((np.abs(got - want)[nlta:] / bound[nlta:]).max())
    print(f"recursive, {n} samples, {-(-n // T)} tiles: {worst:.4f} of twice the bar against the lfilter restatement")
    assert not got[:nlta].any() and np.isfinite(got).all() and worst <= 1.0


@pytest.mark.parametrize("name", list(S.INPUTS))
def test_loud_then_quiet_and_plain(name):
    for nsta, nlta in SMALL:
        for kind in TYPE:
            _check(kind, name, N, nsta, nlta)
            _check(kind, name, N, nsta, nlta, out32=True)


def test_classic_agrees_with_the_cumulative_sum_on_plain_counts():
    """On plain counts (only there) the whole-trace cumulative sum is a yardstick too: the kernel and it agree within the sum
    of the kernel's bar and the running sums' own bound, 2 (i + 1) u S_i per sum, propagated to the ratio."""
    x = S.plain(N)
    for nsta, nlta in SMALL:
        got, want = _run("classic", x, nsta, nlta), S.classic64(x, nsta, nlta)
        t = S.truth("classic", "plain", N, nsta, nlta)
        room = S.bar("classic", t, nsta, nlta).astype(np.float64) + S.cumsum_bound(x, nsta, nlta) * np.abs(want)
        assert (np.abs(got - want) <= room).all() and not want[:nlta - 1].any()


def test_known_answers():
    for nsta, nlta in SMALL:
        lead = nlta + 37
        n = lead + 500
        got = _check("classic", "zeros_then_noise", n, nsta, nlta, lead=lead)
        assert not got[:lead].any() and abs(got[lead] - nlta / nsta) <= (nsta + nlta + 8) * S.U * nlta / nsta
        got = _check("recursive", "zeros_then_noise", n, nsta, nlta, lead=lead)
        assert not got[:lead].any()
        z = np.zeros(3 * nlta + 5000)  # tiny (1 - clta)^i leaves the doubles inside it
        short = S.plain(nlta - 1)
        for kind in TYPE:
            for out32 in (False, True):
                y = _run(kind, z, nsta, nlta, out32=out32)
                assert y.tobytes() == np.zeros(len(z), y.dtype).tobytes()
            assert not _run(kind, short, nsta, nlta + 1).any()  # nlta > n


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_samples(bad):
    n, nsta, nlta = 2 * T + 5, 5, 20
    clean = {kind: _run(kind, S.plain(n), nsta, nlta) for kind in TYPE}
    for at in (0, 7, T - 1, T, T + 1, n - 1):
        x = S.plain(n).copy()
        x[at] = bad
        c = _run("classic", x, nsta, nlta)
        assert np.isnan(c[at:]).all() and np.array_equal(c[:at], clean["classic"][:at])
        r = _run("recursive", x, nsta, nlta)
        if at == 0:  # sample 0 never enters the recursion's sums, whatever it holds
            assert np.array_equal(r, clean["recursive"])
            continue
        first = max(at, nlta)
        assert np.isnan(r[first:]).all() and np.array_equal(r[:first], clean["recursive"][:first])


def _raw(in_t, in_kind, n_series, stride, n, type_, nsta, nlta, out_t, out_kind):
    import torch

    torch.cuda.synchronize()
    return _lib.load().vp_sta_lta(0, C.c_void_p(in_t.data_ptr() if in_t is not None else None), in_kind, n_series, stride, n,
                                  type_, nsta, nlta, C.c_void_p(out_t.data_ptr() if out_t is not None else None), out_kind)


@pytest.mark.parametrize("kind", list(TYPE))
def test_three_series_with_a_stride_equal_three_calls_and_repeat(kind):
    import torch

    n, stride, nsta, nlta = T + 77, T + 200, 50, 1000
    rows = np.zeros((3, stride))
    for k in range(3):
        rows[k, :n] = S.counts(n, 40 + k)
    rows[:, n:] = 1e30  # between the series: never read
    d = _cuda(rows)
    out = torch.full((3, stride), -7.0, dtype=torch.float64, device="cuda")
    assert _raw(d, 2, 3, stride, n, TYPE[kind], nsta, nlta, out, 2) == VP_OK, _lib.last_error()
    again = torch.full((3, stride), -7.0, dtype=torch.float64, device="cuda")
    assert _raw(d, 2, 3, stride, n, TYPE[kind], nsta, nlta, again, 2) == VP_OK
    assert torch.equal(out.view(torch.int64), again.view(torch.int64))  # the same call, the same bits
    got = out.cpu().numpy()
    assert (got[:, n:] == -7.0).all()  # nothing written between the series
    for k in range(3):
        single = _run(kind, rows[k, :n], nsta, nlta)
        assert got[k, :n].tobytes() == single.tobytes()
        assert S.ratio(kind, single, (S.classic_truth if kind == "classic" else S.recursive_truth)(rows[k, :n], nsta, nlta),
                       nsta, nlta) <= 1.0


def test_refusals_leave_out_untouched():
    import torch

    n = 100
    d = _cuda(S.plain(n), np.float32)
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    ok = dict(in_t=d, in_kind=1, n_series=1, stride=n, n=n, type_=1, nsta=5, nlta=20, out_t=out, out_kind=1)
    bad = [dict(in_t=None), dict(out_t=None), dict(in_kind=3), dict(out_kind=0), dict(out_kind=5), dict(type_=2), dict(type_=-1),
           dict(n=-1), dict(n_series=0), dict(stride=n - 1), dict(nsta=0), dict(nsta=21), dict(nlta=0, nsta=0), dict(out_t=d)]
    for change in bad:
        rc = _raw(**dict(ok, **change))
        assert rc == VP_ERR_INVALID and "vp_sta_lta" in _lib.last_error(), change
    assert _raw(**dict(ok, nlta=S.MAX_NLTA + 1)) == VP_ERR_UNSUPPORTED and "65536" in _lib.last_error()
    assert _raw(**dict(ok, n=0, stride=0)) == VP_OK  # n == 0 does nothing
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert _raw(**ok) == VP_OK and not (out.cpu() == -7.0).any()
    assert _raw(**dict(ok, nlta=S.MAX_NLTA, n_series=1)) == VP_OK  # the limit itself works (all zeros: nlta > n)
    assert not out.cpu().numpy().any()
    with pytest.raises(_lib.VolpickHipError, match="65536"):
        TR.sta_lta_device(d, "recstalta", 5, S.MAX_NLTA + 1)
    with pytest.raises(TypeError):
        TR.sta_lta_device(d.to(torch.float16), "recstalta", 5, 20)
    assert TR.release_trigger_scratch(0) > 0 and TR.release_trigger_scratch(0) == 0
    assert _raw(**ok) == VP_OK  # and grows again


def test_a_refused_window_takes_the_host_path_aloud():
    """nlta beyond the kernel's limit: ``Trace.trigger`` and ``sta_lta_triggers`` warn and answer from the host path."""
    n = S.MAX_NLTA + 500
    x = S.bursts(n).astype(np.float32)
    hdr = dict(network="XX", station="A", channel="HHZ", sampling_rate=100.0)
    lta = (S.MAX_NLTA + 1.5) / 100.0
    host = va.Stream([va.Trace(x, hdr)])
    want = va.sta_lta_triggers(host, "recstalta", 5.0, lta)
    dev = va.to_device(host)
    with pytest.warns(UserWarning, match="on the device refused"):
        got = va.sta_lta_triggers(dev, "recstalta", 5.0, lta)
    g, w = got["XX.A..HHZ"], want["XX.A..HHZ"]
    assert isinstance(g["cft"], np.ndarray) and np.array_equal(g["cft"], w["cft"]) and g["on"].tolist() == w["on"].tolist()
    with pytest.warns(UserWarning, match="on the device refused"):
        dev.trigger("recstalta", sta=5.0, lta=lta)
    assert dev[0]._dev is None and np.array_equal(dev[0].data, w["cft"])


def _onset(cft, thr_on, thr_off, per, cap):
    """vp_trigger_onset on a float32 CUDA tensor (n,) or (k, n): (rc, n_found, [(series, on, off, peak, value)])."""
    import torch

    torch.cuda.synchronize()
    k, n = (cft.shape[0], cft.shape[1]) if cft.dim() == 2 else (1, cft.shape[0])
    on, off, pk = (np.full(max(cap, 1), -1, np.int64) for _ in range(3))
    val, ser, found = np.zeros(max(cap, 1), np.float32), np.full(max(cap, 1), -1, np.int32), C.c_int(-1)
    rc = _lib.load().vp_trigger_onset(0, C.c_void_p(cft.data_ptr()), k, n, n, thr_on, thr_off, on.ctypes.data_as(I64),
                                      off.ctypes.data_as(I64), pk.ctypes.data_as(I64), val.ctypes.data_as(C.POINTER(C.c_float)),
                                      ser.ctypes.data_as(C.POINTER(C.c_int32)), per, cap, C.byref(found))
    m = max(min(found.value, cap), 0)
    return rc, found.value, [(int(ser[i]), int(on[i]), int(off[i]), int(pk[i]), float(val[i])) for i in range(m)]


def _mirror(x, thr_on, thr_off):
    return [tuple(v) for v in zip(*TR._pick_host(x, thr_on, thr_off))]


@pytest.mark.parametrize("case", S.TRIGGER_CASES)
def test_trigger_onset_on_the_cft_the_kernel_left(case):
    import torch

    kind, n, nsta, nlta, thr_on, thr_off = case
    x = S.bursts(n)
    rows = np.stack([x, x[::-1], np.roll(x, 1234)])
    cft = TR.sta_lta_device(_cuda(rows), NAME[kind], nsta, nlta, torch.float32)
    host = cft.cpu().numpy()
    want = [_mirror(host[k], thr_on, thr_off) for k in range(3)]
    assert min(len(w) for w in want) > 3
    if case == S.TRIGGER_CASES[-1]:
        assert want[0][-1][1] == n - 1  # a run open at the last sample
    # three series in one call
    rc, found, got = _onset(cft, thr_on, thr_off, 4096, 3 * 4096)
    assert rc == VP_OK and found == sum(len(w) for w in want)
    for k in range(3):
        TC.same([g[1:] for g in got if g[0] == k], want[k])
    assert [g[0] for g in got] == sorted(g[0] for g in got)  # grouped by series, each sorted by onset
    # one series; the public function
    rc, found, got = _onset(cft[0], thr_on, thr_off, 4096, 4096)
    assert rc == VP_OK and found == len(want[0])
    TC.same([g[1:] for g in got], want[0])
    assert TR.trigger_onset(cft[0], thr_on, thr_off).tolist() == [[w[0], w[1]] for w in want[0]]
    # a cap that is too small says so, and the wrapper calls again with more room
    rc, found, _ = _onset(cft, thr_on, thr_off, 2, 3 * 4096)
    assert rc == VP_OK and found > 3 * 4096
    rc, found, _ = _onset(cft, thr_on, thr_off, 4096, 5)
    assert rc == VP_OK and found == sum(len(w) for w in want) > 5
    on, off, pk, val, ser = TR.trigger_onset_device(cft, thr_on, thr_off, cap_per_series=2)
    assert [(int(a), int(b)) for a, b in zip(on[ser == 1], off[ser == 1])] == [(w[0], w[1]) for w in want[1]]


def test_trigger_onset_on_the_adversarial_rows():
    import torch

    z = np.load(ROOT / "tests" / "golden" / "trigger_cases.npz")
    x = torch.from_numpy(z["x"]).cuda()
    for key, thr in (("t_03_03", (0.3, 0.3)), ("t_03_015", (0.3, 0.15)), ("t_05_01", (0.5, 0.1))):
        assert TR.trigger_onset(x, *thr).tolist() == z[key].tolist()
    for pair in TC.PAIRS:
        cases = [c for c in TC.all_cases() if pair in c.pairs and len(c.x) == TC.N]
        assert len(cases) > 300
        cft = torch.from_numpy(np.stack([c.x for c in cases])).cuda()
        rc, found, got = _onset(cft, *pair, TC.N, len(cases) * 64)
        assert rc == VP_OK and found == len(got)
        by_row = {}
        for g in got:
            by_row.setdefault(g[0], []).append(g[1:])
        for k, c in enumerate(cases):
            TC.same(by_row.get(k, []), TC.expected()[(c.name, pair)])
    with pytest.raises(ValueError, match="host path"):
        TR.trigger_onset(x, 0.3, 0.5)
    with pytest.raises(ValueError, match="host path"):
        TR.trigger_onset(x, 0.5, 0.3, max_len=10)
    n = C.c_int(-1)
    lib = _lib.load()
    assert lib.vp_trigger_onset(0, C.c_void_p(x.data_ptr()), 1, 15, 15, 0.3, 0.5, None, None, None, None, None, 0, 0,
                                C.byref(n)) == VP_ERR_INVALID
    assert lib.vp_trigger_onset(0, C.c_void_p(x.data_ptr()), 1, 15, 15, 0.5, 0.3, None, None, None, None, None, 0, 0,
                                C.byref(n)) == VP_OK  # no room at all: the count alone
    assert n.value == len(z["t_05_01"])


@pytest.mark.parametrize("case", S.TRIGGER_CASES)
def test_trace_trigger_and_sta_lta_triggers_against_the_host_path(case):
    import torch

    kind, n, nsta, nlta, thr_on, thr_off = case
    sr = 100.0
    sta, lta = (nsta + 0.5) / sr, (nlta + 0.5) / sr
    hdr = dict(network="XX", station="A", sampling_rate=sr)
    x = S.bursts(n)
    host = va.Stream([va.Trace(x.astype(np.int32), dict(hdr, channel="HHZ")), va.Trace(x[::-1].astype(np.int32), dict(hdr, channel="HHN")),
                      va.Trace(x[:n - 700].astype(np.float32), dict(hdr, channel="HHE"))])
    dev = va.to_device(host)
    got = va.sta_lta_triggers(dev, type=NAME[kind], sta=sta, lta=lta, thr_on=thr_on, thr_off=thr_off)
    want = va.sta_lta_triggers(host, type=NAME[kind], sta=sta, lta=lta, thr_on=thr_on, thr_off=thr_off)
    assert set(got) == set(want) and len(got) == 3
    for tr in host:
        S.clear_of_thresholds(kind, (S.classic_truth if kind == "classic" else S.recursive_truth)(tr.data, nsta, nlta),
                              nsta, nlta, thr_on, thr_off)
        g, w = got[tr.id], want[tr.id]
        assert torch.is_tensor(g["cft"]) and g["cft"].is_cuda and g["cft"].dtype == torch.float32
        assert len(w["on"]) > 3
        for key in ("on", "off", "peak"):
            assert g[key].tolist() == w[key].tolist(), (tr.id, key)
        # both values lie within the float32 bar of the truth at the peak, so within twice that of each other
        rel = (nsta + nlta + 8) * S.U if kind == "classic" else (6 * (w["peak"] + 1.0) + 10) * S.U
        b = (rel + 2.0 ** -24) * np.abs(w["value"].astype(np.float64))
        assert (np.abs(g["value"].astype(np.float64) - w["value"]) <= 2 * b).all()
    # Trace.trigger: in place, on the device, float32
    out = dev.trigger(NAME[kind], sta=sta, lta=lta)
    assert out is dev
    for tr, h in zip(dev, host):
        assert tr._dev is not None and tr._dev.dtype == torch.float32 and tr._data is None
        assert torch.equal(tr._dev, got[tr.id]["cft"])
        t = (S.classic_truth if kind == "classic" else S.recursive_truth)(h.data, nsta, nlta)
        assert S.ratio(kind, tr._dev.cpu().numpy(), t, nsta, nlta, out32=True) <= 1.0
