"""The spectrogram kernel (volpick_amd/csrc/spectrogram.hip) against the float64 restatement and its derived bound
(tests/spectrogram_f64.py; compared with matplotlib's mlab.specgram and shown to have teeth in
tests/test_spectrogram_f64_cpu.py), through the C ABI (``vp_spectrogram``) and the public surface
(``volpick_amd.spectrogram.spectrogram``, ``Trace.spectrogram``, ``Stream.spectrogram``).

Inputs are seeded noise plus a 2 Hz and a 12 Hz burst around an offset (``spectrogram_f64.signal``).  Every case prints its
figure -- the worst |got - want| / bound over the elements; -inf, 0 and NaN must match exactly, else the figure is inf --
before it asserts; LOG.md, "Spectrograms on the device", says which of them have been measured on an MI355X.

On the inputs' means.  The bound's absolute term, 2^-40 A_j, is far below what a mean that differs in its last bits leaks into
the lowest bins (a shift d of the series adds d sum(w) = 64 d to bin 1 at the defaults).  The restatement's numpy mean and
the kernel's fixed-order sum both round; they agree exactly where the sum itself is exact -- int32 counts (below 2^53 in any
order), and float values on a grid of 2^-10 -- and to a few ulps of the offset otherwise, which at the offset of 50 used for
free-running float noise is 1e-14, 60 times under the absolute term."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import spectrogram_f64 as S
from tests import thread_util as TU
from tests.test_spectrogram_f64_cpu import PLANS
from volpick_amd import _lib
from volpick_amd import spectrogram as VS

pytestmark = pytest.mark.gpu

VP_ERR_INVALID, VP_ERR_UNSUPPORTED = -1, -4
TILE = VS.TILE_FRAMES


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: cached inputs are read-only


def _grid(x):
    """Values on a grid of 2^-10: sums of a few million of them are exact in float64 in any order."""
    return np.round(np.asarray(x) * 1024.0) / 1024.0


def _figure(name, got, x, rate, frames=None, **kw):
    """Prints and returns the worst |got - want| / bound of one series' result against the restatement of host array ``x``."""
    want, freq, time, A = S.spectrogram_f64(x, rate, frames=frames, **kw)
    data = got.data.cpu().numpy()
    r = S.ratio(data, want, A, kw.get("dbscale", False))
    print(f"{name}: {data.shape}, worst |got - want| / bound = {r:.3e}")
    assert data.dtype == np.float32 and np.array_equal(got.freq, freq) and np.array_equal(got.time, time)
    return r


def _raw(x_dev, n_series, stride, n, rate, nfft, pad, hop, db, first, count, out, kind=None):
    return _lib.load().vp_spectrogram(0, C.c_void_p(x_dev.data_ptr() if x_dev is not None else None),
                                      VS.SAMPLE_KINDS[str(x_dev.dtype)] if kind is None else kind, n_series, stride, n, rate, nfft, pad,
                                      hop, db, first, count, C.c_void_p(out.data_ptr() if out is not None else None), None)


@functools.lru_cache(maxsize=None)
def _default_case():
    x = S.signal(3001, 31).astype(np.float32)
    x.setflags(write=False)
    return x, VS.spectrogram(_cuda(x), 100.0)


# ------------------------------------------------------------------------------------------ 1. defaults
def test_defaults_float32_3001_samples():
    x, got = _default_case()
    assert tuple(got.data.shape) == (512, 222) and got.data.is_cuda
    assert _figure("defaults, float32, 3001 samples", got, x, 100.0) <= 1.0


# ------------------------------------------------------------------------------------------ 2. the frame tile
def test_every_frame_count_from_2_to_two_tiles_and_one():
    nfft, hop = 128, 13
    base = _grid(S.signal(nfft + hop * (2 * TILE + 1), 32)).astype(np.float32)
    worst = 0.0
    for n_frames in range(2, 2 * TILE + 2):
        x = base[: nfft + hop * (n_frames - 1)]
        got = VS.spectrogram(_cuda(x), 100.0)
        assert tuple(got.data.shape) == (512, n_frames)
        want, _, _, A = S.spectrogram_f64(x, 100.0)
        r = S.ratio(got.data.cpu().numpy(), want, A)
        assert r <= 1.0, f"{n_frames} frames: {r:.3e}"
        worst = max(worst, r)
    print(f"n_frames 2 .. {2 * TILE + 1} (tile {TILE}): worst |got - want| / bound = {worst:.3e}")
    # hop - 1 dangling samples behind the last frame change nothing but the mean
    x = base[: nfft + hop * TILE + hop - 1]
    got = VS.spectrogram(_cuda(x), 100.0)
    assert tuple(got.data.shape) == (512, TILE + 1)
    assert _figure(f"{TILE + 1} frames and {hop - 1} dangling samples", got, x, 100.0) <= 1.0


# ------------------------------------------------------------------------------------------ 3. kinds
@pytest.mark.parametrize("kind", ("int32", "float64", "float32"))
def test_sample_kinds(kind):
    if kind == "int32":  # counts of amplitude 10 around 1e6: a float32 mean is off by up to 1 / 32 there
        x = np.round(S.signal(3001, 33, offset=1e6)).astype(np.int32)
    elif kind == "float64":  # an offset of 2^24 + 1 and steps of 2^-10: float32 holds neither
        x = _grid(S.signal(3001, 34, offset=0.0)) + 16777217.0
        assert not np.array_equal(x.astype(np.float32).astype(np.float64), x)
    else:
        x = S.signal(3001, 35).astype(np.float32)
    got = VS.spectrogram(_cuda(x), 100.0)
    assert _figure(kind, got, x, 100.0) <= 1.0


# ------------------------------------------------------------------------------------------ 4. plans
MORE_PLANS = {
    "512 / 4096 (the cap)": (12000, 100.0, {"wlen": 5.12}),
    "per_lap 0.99 (hop 2)": (1001, 100.0, {"per_lap": 0.99}),
    "nfft 32": (1001, 100.0, {"wlen": 0.32}),
    "nfft 32, mult 16": (1001, 100.0, {"wlen": 0.32, "mult": 16.0}),
    "nfft 64, per_lap 0": (2000, 100.0, {"wlen": 0.64, "per_lap": 0.0}),
    "nfft 256, mult 16, dbscale": (6000, 100.0, {"wlen": 2.56, "mult": 16.0, "dbscale": True}),
    "nfft 512, per_lap 0, mult None": (12000, 100.0, {"wlen": 5.12, "per_lap": 0.0, "mult": None}),
    "50 Hz": (3001, 50.0, {}),
    "200 Hz": (3001, 200.0, {}),
    "250 Hz": (3001, 250.0, {}),
}
ALL_PLANS = {**PLANS, **MORE_PLANS}


@pytest.mark.parametrize("name", list(ALL_PLANS))
def test_plans(name):
    npts, rate, kw = ALL_PLANS[name]
    x = S.signal(npts, 36, rate).astype(np.float32)
    got = VS.spectrogram(_cuda(x), rate, **kw)
    nfft, pad, _, _, n_frames = S.plan(npts, rate, kw.get("per_lap", 0.9), kw.get("wlen"), kw.get("mult", 8.0))
    assert tuple(got.data.shape) == (pad // 2, n_frames)
    assert _figure(f"{name} (nfft {nfft}, pad {pad})", got, x, rate, **kw) <= 1.0


def test_one_frame_of_128_samples_through_the_c_entry():
    """The reference (and ``spectrogram()``) refuse fewer than two frames; the C entry computes the one frame."""
    import torch

    x = S.signal(128, 37).astype(np.float32)
    with pytest.raises(ValueError):
        VS.spectrogram(_cuda(x), 100.0)
    out = torch.full((512, 1), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_raw(_cuda(x), 1, 128, 128, 100.0, 128, 1024, 13, 0, 0, 1, out), "vp_spectrogram")
    amp = S._amplitudes(x, 100.0, 128, 1024, 13, (0, 1))
    r = S.ratio(out.cpu().numpy(), amp[1:], amp.max(axis=0))
    print(f"one frame of 128 samples: worst |got - want| / bound = {r:.3e}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------ 5. dbscale and zeros
@pytest.mark.parametrize("dbscale", (True, False))
def test_a_stretch_of_exact_zeros_longer_than_a_frame(dbscale):
    v = np.round(S.signal(1200, 38, offset=0.0))
    x = np.concatenate([v, np.zeros(400), -v]).astype(np.int32)  # the mean is exactly 0
    got = VS.spectrogram(_cuda(x), 100.0, dbscale=dbscale)
    data = got.data.cpu().numpy()
    want = S.spectrogram_f64(x, 100.0, dbscale=dbscale)[0]
    zero = np.isneginf(want).all(axis=0) if dbscale else (want == 0).all(axis=0)
    assert zero.sum() >= 20
    assert (np.isneginf(data[:, zero]) if dbscale else data[:, zero] == 0).all() and np.isfinite(data[:, ~zero]).all()
    assert _figure(f"zeros, dbscale {dbscale} ({zero.sum()} columns)", got, x, 100.0, dbscale=dbscale) <= 1.0


# ------------------------------------------------------------------------------------------ 6. non-finite input
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("dbscale", (False, True))
def test_one_nan_or_inf_makes_the_whole_output_nan(value, dbscale):
    x = S.signal(3001, 39).astype(np.float32)
    x[2900] = value
    block = np.stack([x, S.signal(3001, 40).astype(np.float32)])
    got = VS.spectrogram(_cuda(block), 100.0, dbscale=dbscale).data.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()  # the series beside it is untouched


# ------------------------------------------------------------------------------------------ 7. - 9. bit-identical forms
def test_a_block_in_one_call_equals_three_single_calls_bit_for_bit():
    import torch

    block = np.stack([S.signal(3001, 41 + c, offset=50.0 * c) for c in range(3)]).astype(np.float32)
    d = _cuda(block)
    whole = VS.spectrogram(d, 100.0)
    assert tuple(whole.data.shape) == (3, 512, 222)
    singles = [VS.spectrogram(d[c], 100.0).data for c in range(3)]
    assert torch.equal(whole.data.view(torch.int32), torch.stack(singles).view(torch.int32))
    assert _figure("series 2 of the block", VS.Spectrogram(whole.data[2], whole.freq, whole.time), block[2], 100.0) <= 1.0
    # the same series at a stride above N, and a (2, 3, N) bank tensor
    wide = torch.zeros((3, 3001 + 7), dtype=torch.float32, device="cuda")
    wide[:, :3001] = d
    assert torch.equal(VS.spectrogram(wide[:, :3001], 100.0).data.view(torch.int32), whole.data.view(torch.int32))
    bank = torch.stack([d, d.flip(0)])
    got = VS.spectrogram(bank, 100.0).data
    assert tuple(got.shape) == (2, 3, 512, 222)
    assert torch.equal(got[0].view(torch.int32), whole.data.view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), whole.data.flip(0).view(torch.int32))
    for bad in (d[:, ::2], d.t(), bank[:, ::2, :].transpose(0, 1)[:, :, :], d.to(torch.float16), d.cpu()):
        with pytest.raises((TypeError, ValueError)):
            VS.spectrogram(bad, 100.0)


def test_a_frame_range_equals_the_slice_of_the_full_result_bit_for_bit():
    import torch

    x, full = _default_case()
    d = _cuda(x)
    for lo, hi in ((0, 1), (0, TILE), (5, 77), (TILE - 1, TILE + 1), (2 * TILE, 222), (221, 222), (100, 100)):
        part = VS.spectrogram(d, 100.0, frames=(lo, hi))
        assert tuple(part.data.shape) == (512, hi - lo)
        assert torch.equal(part.data.view(torch.int32), full.data[:, lo:hi].contiguous().view(torch.int32)), (lo, hi)
        assert np.array_equal(part.time, full.time[lo:hi]) and np.array_equal(part.freq, full.freq)
    with pytest.raises(ValueError):
        VS.spectrogram(d, 100.0, frames=(0, 223))


def test_the_same_call_twice_gives_identical_bits():
    import torch

    x, first = _default_case()
    again = VS.spectrogram(_cuda(x), 100.0)
    assert torch.equal(first.data.view(torch.int32), again.data.view(torch.int32))


# ------------------------------------------------------------------------------------------ 10. a long series
def test_a_million_and_three_counts_in_three_frame_ranges():
    """The chunked mean (62 blocks) and 64-bit offsets, without a gigabyte of output."""
    n = 1_000_003
    rng = np.random.default_rng(42)
    x = (rng.standard_normal(n) * 300.0 + 1_234_567.0).round().astype(np.int32)
    t = np.arange(600) / 100.0
    for at, hz in ((TILE * 13 * 1200 - 100, 2.0), (n - 2000, 12.0)):
        x[at : at + 600] += (4000.0 * np.exp(-t / 1.5) * np.sin(2 * np.pi * hz * t)).astype(np.int32)
    d = _cuda(x)
    total = S.plan(n, 100.0)[4]
    assert total == 76914
    for lo, hi in ((0, 40), (TILE * 1200 - 10, TILE * 1200 + 10), (total - 35, total)):
        got = VS.spectrogram(d, 100.0, frames=(lo, hi))
        assert _figure(f"frames [{lo}, {hi}) of {total}", got, x, 100.0, frames=(lo, hi)) <= 1.0


# ------------------------------------------------------------------------------------------ 11. the public surface
def test_traces_and_streams():
    import torch

    import volpick_amd as va

    x = np.stack([np.round(S.signal(3001, 50 + c, offset=5000.0)) for c in range(3)]).astype(np.int32)
    t0 = va.UTCDateTime("2020-01-01T00:00:00")
    st = va.Stream([va.Trace(x[c].copy(), {"network": "XX", "station": "SPEC", "channel": "HH" + comp, "starttime": t0,
                                           "sampling_rate": 100.0}) for c, comp in enumerate("ZNE")])
    moved = va.to_device(st)
    on_device = moved.spectrogram(dbscale=True)
    on_host = st.spectrogram(dbscale=True)
    assert len(on_device) == len(on_host) == 3
    assert all(tr._dev is not None and tr._data is None for tr in moved)  # never copied back
    for c in range(3):
        assert isinstance(on_device[c], va.Spectrogram) and on_device[c].data.is_cuda and on_host[c].data.is_cuda
        assert torch.equal(on_device[c].data.view(torch.int32), on_host[c].data.view(torch.int32))
        assert _figure(f"trace {c} (dbscale)", on_device[c], x[c], 100.0, dbscale=True) <= 1.0
    one = moved[1].spectrogram(frames=(3, 9), per_lap=0.5)
    assert tuple(one.data.shape) == (512, 6) and moved[1]._data is None
    assert _figure("trace 1, frames [3, 9), per_lap 0.5", one, x[1], 100.0, frames=(3, 9), per_lap=0.5) <= 1.0
    assert torch.equal(va.spectrogram.spectrogram(moved[1], per_lap=0.5, frames=(3, 9)).data, one.data)
    masked = va.Trace(x[0].astype(np.float32), {"sampling_rate": 100.0})
    masked._data = np.ma.masked_array(masked._data, mask=np.arange(3001) == 7)  # what a gappy merge leaves in an ObsPy trace
    with pytest.raises(NotImplementedError):
        masked.spectrogram()
    with pytest.raises(ValueError):
        va.Trace(x[0][:127], {"sampling_rate": 100.0}).spectrogram()


# ------------------------------------------------------------------------------------------ 12. refusals
GOOD = dict(n_series=1, stride=3001, n=3001, rate=100.0, nfft=128, pad=1024, hop=13, db=0, first=0, count=222)
REFUSALS = {
    "unknown kind": (VP_ERR_INVALID, dict(kind=3)),
    "n < nfft": (VP_ERR_INVALID, dict(n=127, stride=127, count=0)),
    "hop 0": (VP_ERR_INVALID, dict(hop=0)),
    "hop > nfft": (VP_ERR_INVALID, dict(hop=129)),
    "nfft not a power of two": (VP_ERR_INVALID, dict(nfft=100)),
    "pad not a power of two": (VP_ERR_INVALID, dict(pad=1000)),
    "pad < nfft": (VP_ERR_INVALID, dict(pad=64)),
    "one frame too many": (VP_ERR_INVALID, dict(count=223)),
    "a negative first frame": (VP_ERR_INVALID, dict(first=-1, count=1)),
    "a range past the end": (VP_ERR_INVALID, dict(first=222, count=1)),
    "series_stride < n": (VP_ERR_INVALID, dict(stride=3000)),
    "samp_rate 0": (VP_ERR_INVALID, dict(rate=0.0)),
    "samp_rate negative": (VP_ERR_INVALID, dict(rate=-100.0)),
    "samp_rate NaN": (VP_ERR_INVALID, dict(rate=float("nan"))),
    "samp_rate inf": (VP_ERR_INVALID, dict(rate=float("inf"))),
    "nfft 16": (VP_ERR_UNSUPPORTED, dict(nfft=16, pad=128, hop=2, count=10)),
    "nfft 1024": (VP_ERR_UNSUPPORTED, dict(nfft=1024, pad=1024, hop=103, count=10)),
    "pad / nfft 32": (VP_ERR_UNSUPPORTED, dict(nfft=32, pad=1024, hop=4, count=10)),
    "pad 8192": (VP_ERR_UNSUPPORTED, dict(nfft=512, pad=8192, hop=52, count=10)),
}


@functools.lru_cache(maxsize=None)
def _refusal_buffers():
    import torch

    return _cuda(S.signal(3001, 60).astype(np.float32)), torch.full((512, 222), -7.0, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("name", ["null input", "null output"] + list(REFUSALS))
def test_every_refusal_names_the_entry_point_and_leaves_the_output_untouched(name):
    x, out = _refusal_buffers()
    a = dict(GOOD)
    if name.startswith("null"):
        want = VP_ERR_INVALID
        rc = _raw(None if name == "null input" else x, out=None if name == "null output" else out, kind=1,
                  **{k: a[k] for k in ("n_series", "stride", "n", "rate", "nfft", "pad", "hop", "db", "first", "count")})
    else:
        want, change = REFUSALS[name]
        a.update(change)
        kind = a.pop("kind", None)
        rc = _raw(x, out=out, kind=kind, **a)
    msg = _lib.last_error()
    print(f"{name}: rc = {rc}, message = {msg!r}")
    assert rc == want and "vp_spectrogram" in msg
    assert bool((out == -7.0).all())
    if want == VP_ERR_UNSUPPORTED:
        assert "512" in msg and "4096" in msg and "16" in msg  # the limits
    if name == "nfft 1024":
        with pytest.raises(_lib.VolpickHipError):
            VS.spectrogram(x, 100.0, wlen=10.24)


# ------------------------------------------------------------------------------------------ 13. host threads
def test_two_host_threads_and_a_release_between_calls():
    import torch

    TU.check_not_stuck()
    xs = [_cuda(S.signal(3001 + 500 * i, 70 + i).astype(np.float32)) for i in range(2)]
    kws = [dict(), dict(wlen=2.56, dbscale=True)]
    alone = [VS.spectrogram(xs[i], 100.0, **kws[i]).data.clone() for i in range(2)]
    rounds = 6

    def worker(i):
        def run():
            torch.cuda.set_device(0)
            return [VS.spectrogram(xs[i], 100.0, **kws[i]).data for _ in range(rounds)]
        return run

    results, wall = TU.run_threads([worker(0), worker(1)], names=["defaults", "wlen 2.56 dbscale"])
    for i in range(2):
        for got in results[i]:
            assert torch.equal(got.view(torch.int32), alone[i].view(torch.int32))
    TU.report("spectrogram on two threads", 2, rounds, wall)
    freed = VS.release_spectrogram_scratch(0)
    assert freed > 0 and VS.release_spectrogram_scratch(0) == 0
    for i in range(2):
        assert torch.equal(VS.spectrogram(xs[i], 100.0, **kws[i]).data.view(torch.int32), alone[i].view(torch.int32))
