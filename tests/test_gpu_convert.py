"""GPU: event files to a waveform bank without a host visit -- ``read_many`` against ``read``, ``trim`` on device traces,
``vp_bank_assemble`` against the extended-precision truth at the bar tests/convert_restate.py derives, its refusals, and
``bank_from_streams`` against the host route (``detrend("demean")``, ``io.stream_to_array``, ``WaveformBank(list, onsets)``).

The assembly kernels work in tiles of ``VP_ASSEMBLE_TILE`` = AS_NTH * AS_PER = 256 * 16 = 4096 samples (csrc/assemble.hip: a
workgroup's share of a piece's mean range in the sums, and of a row in the store); the shapes below sit on that tile's edges."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import convert_restate as R
from tests.mseed_util import T0, file_bytes, seismogram
from tests.test_convert_cpu import make, us
from volpick_amd import _lib, generate
from volpick_amd import io as vio
from volpick_amd._device import SAMPLE_KINDS
from volpick_amd.stream import UTCDateTime

pytestmark = pytest.mark.gpu

T = _lib.VP_ASSEMBLE_TILE
VP_ERR_INVALID = -1


# ---------------------------------------------------------------------------------------------------------- read_many
def _files():
    rng = np.random.default_rng(17)
    x = seismogram(4000, rng)
    hdr = dict(network="XX", station="EVT", location="", rate=100.0)
    steim = file_bytes([dict(hdr, channel="HH" + c, start_us=T0, data=seismogram(2500, rng)) for c in "ZNE"])
    gappy = file_bytes([dict(hdr, channel="HHZ", start_us=T0, data=x[:1500]),
                        dict(hdr, channel="HHZ", start_us=T0 + 20_000_000, data=x[1500:]),   # 5 s gap
                        dict(hdr, channel="HHN", start_us=T0 + 290_000, data=x[:900])], encoding=3)
    floats = file_bytes([dict(hdr, channel="HH" + c, start_us=T0 + 570_000, data=rng.standard_normal(1200).astype(np.float32))
                         for c in "ZE"], encoding=4)
    return [steim, gappy, floats]


def test_read_many_matches_read_with_one_decode_per_kind(lib, monkeypatch):
    import torch

    files = _files()
    calls = []
    real = lib.vp_mseed_decode
    monkeypatch.setattr(lib, "vp_mseed_decode", lambda *a: (calls.append(a[8]), real(*a))[1])
    want = [vio.read(f, device_resident=True) for f in files]
    assert len(calls) == 3  # one per file (each holds one sample kind)
    del calls[:]
    got = vio.read_many(files)
    assert sorted(calls) == [_lib.VP_SAMPLES_INT32, _lib.VP_SAMPLES_FLOAT32]  # one launch per sample kind for all files
    assert [len(s) for s in got] == [len(s) for s in want] == [3, 3, 2]
    for sg, sw in zip(got, want):
        for a, b in zip(sg, sw):
            assert dict(a.stats) == dict(b.stats) and a.id == b.id
            assert a._dev.is_cuda and a._dev.dtype == b._dev.dtype and torch.equal(a._dev, b._dev)
    ints = [tr._dev for s in got for tr in s if tr._dev.dtype == torch.int32]
    assert len({t.untyped_storage().data_ptr() for t in ints}) == 1  # views into one shared decode buffer
    # a short payload is named with the offset within its own file, as read() names it
    bad = bytearray(files[1])
    n2 = int(vio.scan_mseed(files[1])["nsamples"][2])
    bad[2 * 512 + 30: 2 * 512 + 32] = (n2 + 900).to_bytes(2, "big")
    with pytest.raises(ValueError) as e_read:
        vio.read(bytes(bad), device_resident=True)
    with pytest.raises(ValueError) as e_many:
        vio.read_many([files[0], bytes(bad), files[2]])
    assert str(e_many.value) == str(e_read.value) and "fewer samples" in str(e_many.value)


# --------------------------------------------------------------------------------------------------------------- trim
def test_trim_on_device_traces():
    from volpick_amd import to_device

    _, st = make([("HHZ", 0.0, 5000), ("HHN", 0.29, 3000), ("HHE", 40.0, 100)], seed=3)
    dev = to_device(st)
    full = [tr._dev for tr in dev]
    t0, t1 = st[0].stats.starttime + 10.004, st[0].stats.starttime + 35.506
    host = st.copy().trim(t0, t1)
    assert dev.trim(t0, t1) is dev and len(dev) == len(host) == 2
    for tr, h, f in zip(dev, host, full):
        assert tr._dev is not None and tr._dev.is_cuda and tr._data is None
        assert tr._dev.untyped_storage().data_ptr() == f.untyped_storage().data_ptr()  # a view: no copy
        assert dict(tr.stats) == dict(h.stats)
        first = (tr._dev.data_ptr() - f.data_ptr()) // f.element_size()
        assert first > 0 and np.array_equal(tr._dev.cpu().numpy(), h.data)
        assert np.array_equal(f[first:first + len(tr)].cpu().numpy(), h.data)


# ----------------------------------------------------------------------------------------------------------- assembly
def _piece(x, c, dst=0, keep_lo=0, keep_n=None):
    return dict(x=x, component=c, keep_lo=keep_lo, keep_n=len(x) - keep_lo if keep_n is None else keep_n, dst=dst)


def _events():
    """[(L, pieces in table order)]: the shapes of the module docstring."""
    rng = np.random.default_rng(2024)

    def i32(n, scale=20000):
        return (rng.integers(-scale, scale, n) + 1234).astype(np.int32)

    def f32(n):
        return (rng.standard_normal(n) * 3000 + 50).astype(np.float32)

    def f64(n):
        return rng.standard_normal(n) * 1e4 - 77.7

    ev = []
    for L in (1, 2, T - 1, T, T + 1, 3 * T + 5):  # the tile's edges and a few tiles; the three kinds mixed in every event
        ev.append((L, [_piece(i32(L), 0), _piece(f32(L), 1), _piece(f64(L), 2)]))
    ev.append((1, [_piece(i32(5), 0, keep_lo=3, keep_n=1), _piece(f64(2), 2, keep_lo=1, keep_n=1)]))
    ev.append((300, [_piece(i32(300), 0), _piece(f32(300), 2)]))      # two components
    ev.append((T + 7, [_piece(f64(T + 7), 1)]))                       # one component
    ev.append((50, []))                                               # none
    for c, kinds in ((0, (i32, i32)), (1, (f32, f64)), (2, (f64, i32))):
        a, b = kinds
        ev.append((1000, [_piece(a(200), c, 300), _piece(b(1000), c)]))       # shorter first: the longer one hides it
        ev.append((1000, [_piece(b(1000), c), _piece(a(200), c, 300)]))       # longer first: the short one lies inside it and wins
        ev.append((1000, [_piece(a(600), c), _piece(b(600), c, 400)]))        # equal lengths
    ev.append((1000, [_piece(i32(300), 0, 100), _piece(f32(500), 0, 350), _piece(f64(700), 0, 300), _piece(i32(1000), 1)]))
    ev.append((2 * T, [_piece(i32(T + 100), 2), _piece(f32(T + 100), 2, T - 100)]))  # an overlap across a tile boundary
    x = i32(1500)
    x[:500] += 100000  # the kept range's own mean differs from the mean range's by about 33000
    ev.append((700, [_piece(x, 1, keep_lo=500, keep_n=700)]))
    ev.append((20, [_piece(f64(2 * T + 3), 0, dst=5, keep_lo=T - 1, keep_n=10)]))  # a mean range of several tiles, little kept
    big = rng.choice(np.array([2 ** 31 - 1, -2 ** 31, 2 ** 31 - 5, -2 ** 31 + 3], np.int64), T + 1).astype(np.int32)
    ev.append((T + 1, [_piece(big, 0), _piece(big[::-1].copy(), 2, keep_lo=1)]))
    ev.append((T + 1, [_piece(np.full(T + 1, 12345, np.int32), 0), _piece(np.full(T + 1, -0.5, np.float32), 1),
                       _piece(np.full(2 * T, 7.0), 2, keep_lo=9, keep_n=T + 1)]))  # constant traces alone in their rows
    while len(ev) < 40:
        L = int(rng.integers(1, 2 * T))
        pcs = []
        for c in range(3):
            for _ in range(int(rng.integers(0, 4))):
                n = int(rng.integers(1, L + 200))
                keep_n = int(rng.integers(1, min(n, L) + 1))
                pcs.append(_piece((i32, f32, f64)[int(rng.integers(3))](n), c, int(rng.integers(0, L - keep_n + 1)),
                                  int(rng.integers(0, n - keep_n + 1)), keep_n))
        ev.append((L, pcs))
    return ev


def _table(events, first_trace=0):
    """(ASSEMBLE_PIECE array, the device tensors it points into, lengths)."""
    import torch

    rows, keep = [], []
    for i, (L, pcs) in enumerate(events):
        for pc in pcs:
            t = torch.from_numpy(np.ascontiguousarray(pc["x"])).cuda()
            keep.append(t)
            rows.append((t.data_ptr(), len(pc["x"]), pc["keep_lo"], pc["keep_n"], pc["dst"], first_trace + i, pc["component"],
                         SAMPLE_KINDS[str(t.dtype)], 0))
    return np.array(rows, generate.ASSEMBLE_PIECE), keep, np.array([L for L, _ in events], np.int64)


@pytest.fixture(scope="module")
def assembled():
    events = _events()
    assert len(events) == 40 and all(pcs == sorted(pcs, key=lambda p: p["component"]) for _, pcs in events)
    pieces, keep, lengths = _table(events)
    onsets = {"P": np.full(len(events), np.nan), "S": np.full(len(events), np.nan)}
    bank = generate.WaveformBank.from_pieces(pieces, lengths, onsets, sources=keep)  # one vp_bank_assemble call
    got = [bank.trace(i) for i in range(len(events))]
    truth = [R.assemble_truth(L, pcs) for L, pcs in events]
    return types.SimpleNamespace(events=events, pieces=pieces, keep=keep, lengths=lengths, onsets=onsets, bank=bank, got=got,
                                 truth=truth)


def test_assembled_values_meet_the_derived_bar(assembled):
    worst = 0.0
    for i, (got, (truth, bar)) in enumerate(zip(assembled.got, assembled.truth)):
        assert got.shape == truth.shape and got.dtype == np.float32
        r = R.worst_ratio(got, truth, bar)
        print(f"event {i}: L = {got.shape[1]}, worst |got - truth| / bar = {r:.3f}")
        worst = max(worst, r)
    assert worst <= 1.0, f"worst |got - truth| / bar = {worst}"


def test_exact_zeros_and_repeatability(assembled):
    n_zero_rows = 0
    for got, (truth, _), (L, pcs) in zip(assembled.got, assembled.truth, assembled.events):
        for c in range(3):
            if not np.any(truth[c]):  # a row without a trace, or a constant trace alone in its row
                n_zero_rows += 1
                assert not np.any(got[c]), "a row whose truth is exactly 0 is not exactly 0"
    assert n_zero_rows >= 12
    again = generate.WaveformBank.from_pieces(assembled.pieces, assembled.lengths, assembled.onsets, sources=assembled.keep)
    for i, got in enumerate(assembled.got):
        assert np.array_equal(again.trace(i).view(np.uint32), got.view(np.uint32)), f"trace {i} differs between two runs"
    again.close()


def test_refusals_leave_the_bank_untouched(lib, assembled):
    import torch

    events = assembled.events[7:9]
    L0, L1 = (L for L, _ in events)
    h = C.c_void_p()
    _lib.check(lib.vp_bank_create(0, 2, int(3 * (L0 + L1)), C.byref(h)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan4 = np.full(4, np.nan)

    def call(pieces, first, lens, n=1):
        lens = np.asarray(lens, np.int64)
        return lib.vp_bank_assemble(h, first, n, pieces.ctypes.data_as(C.c_void_p), len(pieces),
                                    lens.ctypes.data_as(C.POINTER(C.c_int64)), np.tile(nan4, n).ctypes.data_as(C.POINTER(C.c_double)),
                                    stream)

    def read(i, L):
        out = np.empty((3, L), np.float32)
        _lib.check(lib.vp_bank_read(h, i, out.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST))
        return out

    p0, keep0, _ = _table(events[:1])
    assert call(p0, 0, [L0]) == 0
    before = read(0, L0)
    assert np.array_equal(before, assembled.got[7])
    good, keep1, _ = _table(events[1:], first_trace=1)
    assert len(good) == 1 and good["keep_n"][0] == L1

    def bad(**fields):
        p = good.copy()
        for k, v in fields.items():
            p[k] = v
        return p

    cases = {
        "trace outside the bank": (bad(trace=5), 1, [L1]),
        "trace outside the call": (bad(trace=0), 1, [L1]),
        "traces out of order (again)": (bad(trace=0), 0, [L1]),
        "traces out of order (ahead)": (bad(trace=2), 2, [L1]),
        "past the bank's traces": (good, 1, [L1, 1], 2),
        "past the bank's floats": (good, 1, [L1 + 1]),
        "piece past its row": (bad(dst=1), 1, [L1]),
        "piece before its row": (bad(dst=-1, keep_n=5), 1, [L1]),
        "kept range past its mean range": (bad(keep_lo=1), 1, [L1]),
        "kept range before its mean range": (bad(keep_lo=-1, keep_n=5), 1, [L1]),
        "trace length 0": (good[:0], 1, [0]),
        "mean range of 0": (bad(mean_n=0), 1, [L1]),
        "kept range of 0": (bad(keep_n=0), 1, [L1]),
        "unknown sample kind": (bad(kind=3), 1, [L1]),
        "component 3": (bad(component=3), 1, [L1]),
        "null source": (bad(src=0), 1, [L1]),
        "rows descending": (np.concatenate([bad(component=2, keep_n=3), bad(component=1, keep_n=3)]), 1, [L1]),
    }
    for name, args in cases.items():
        assert call(*args) == VP_ERR_INVALID, name
        assert b"vp_bank_assemble" in lib.vp_last_error(), name
        assert lib.vp_bank_read(h, 1, before.ctypes.data_as(C.c_void_p), _lib.VP_MEM_HOST) == VP_ERR_INVALID, name  # nothing written
    assert np.array_equal(read(0, L0), before)
    assert call(good, 1, [L1]) == 0  # the bank still takes its next trace
    assert np.array_equal(read(1, L1), assembled.got[8]) and np.array_equal(read(0, L0), before)
    _lib.check(lib.vp_bank_destroy(h))


# ------------------------------------------------------------------------------------- equivalence with the host route
SPECS = [
    [("HHZ", 0.0, 3000), ("HHN", 0.29, 2900), ("HHE", 0.57, 2800)],
    [("HHZ", 5.0, 400), ("HHZ", 0.0, 3000), ("HHN", 0.0, 3000), ("HHE", 0.0, 2000), ("HHE", 15.0, 2000)],
    [("EHZ", 0.0, 2500), ("EHE", 0.58, 2500)],
    [("HHZ", 0.0, 4200), ("HHN", 0.01, 4199), ("HHE", 0.0, 4100), ("EHZ1", 0.0, 100)],
]
P_S = [(8.0, 14.0), (10.0, None), (None, 9.5), (12.34, 20.0)]


def _old_bar(truth, pieces, L):
    """The host route's own bar, by the reasoning of convert_restate.py: numpy's float64 piece mean (N_w terms), x - m, the
    row mean as one sum of L values <= 2 X, the subtraction, then fp32: d64 = u X (N_w + 2 + 2 L + 4)."""
    bar = np.zeros_like(truth)
    for c in range(3):
        row = [p for p in pieces if p["component"] == c]
        if not row:
            continue
        X = max(float(np.abs(p["x"].astype(np.float64)).max()) for p in row)
        n_w = np.zeros(L)
        for p in row:
            n_w[p["dst"]:p["dst"] + p["keep_n"]] = len(p["x"])
        d64 = R.U * X * (n_w + 2 + 2 * L + 4)
        bar[c] = 2.0 ** -24 * (np.abs(truth[c]) + d64) + d64
    return bar


def test_bank_from_streams_matches_the_host_route():
    import torch

    from volpick_amd import bank_from_streams, plan_event

    made = [make(s, seed=40 + i) for i, s in enumerate(SPECS)]
    for i, (dicts, st) in enumerate(made):  # mixed sample kinds
        for j, tr in enumerate(st):
            if (i + j) % 3 == 1:
                tr.data = (tr.data * 1.37).astype(np.float32)
                dicts[j]["data"] = tr.data
    streams = [st for _, st in made]
    base = streams[0][0].stats.starttime  # every offset of SPECS and P_S counts from here
    p_times = [None if p is None else str(base + p) for p, _ in P_S]
    s_times = [None if s is None else str(base + s) for _, s in P_S]
    meta = {"trace_p_arrival_time": p_times, "trace_s_arrival_time": s_times}
    bank, table = bank_from_streams(streams, meta)

    # the table against the restatement, exactly
    for i, ((dicts, st), (p, s)) in enumerate(zip(made, P_S)):
        want = R.restate_event(dicts, us(p), us(s))
        assert table["trace_npts"][i] == want["samples"] == bank.lengths[i]
        assert table["trace_start_time"][i] == str(UTCDateTime._from_us(want["start_us"]))
        assert table["trace_completeness"][i] == want["completeness"] and table["trace_sampling_rate_hz"][i] == 100
        for name, v in (("p", want["p_sample"]), ("s", want["s_sample"])):
            got = table[f"trace_{name}_arrival_sample"][i]
            assert (np.isnan(got) and v is None) or got == v
    assert np.array_equal(bank.onsets[:, 0], table["trace_p_arrival_sample"], equal_nan=True)
    assert np.array_equal(bank.onsets[:, 2], table["trace_s_arrival_sample"], equal_nan=True)

    # the host route of the parent commit
    arrays = [vio.stream_to_array(st.copy().detrend("demean"))[1] for st in streams]
    old = generate.WaveformBank(arrays, {"P": table["trace_p_arrival_sample"], "S": table["trace_s_arrival_sample"]})

    # plan rows: a window hanging over the start, one over the end, one inside, per trace
    Tw = 1024
    model = types.SimpleNamespace(in_samples=Tw, labels="PSN", norm="peak")
    rows = np.zeros(3 * len(streams), generate.PLAN_ROW)
    for i, L in enumerate(bank.lengths):
        rows["trace"][3 * i:3 * i + 3] = i
        rows["start"][3 * i:3 * i + 3] = (-300, L - 700, 500)
        rows["hi"][3 * i:3 * i + 3] = L
    new_b, old_b = bank.make_batch(rows, model, 20), old.make_batch(rows, model, 20)
    assert torch.equal(new_b["y"], old_b["y"])  # the same onsets through the same kernel
    xn, xo = new_b["X"].cpu().numpy().astype(np.float64), old_b["X"].cpu().numpy().astype(np.float64)

    # The bar.  Both banks lie within their own bar of the truth, so they differ by at most e = bar_new + bar_old per
    # sample.  A window's mean then moves by at most e_w = max e over the window, a = w - mean by 2 e_w, the peak
    # D = max|a| + 1e-10 by 2 e_w, and q = a / D with |q| <= 1 by (2 e_w + |q| 2 e_w) / D' <= 4 e_w / (D - 2 e_w); each
    # kernel run rounds its q once to fp32 (2^-24 each) on float64 statistics (1e-12 covers them).
    worst = 0.0
    for i, st in enumerate(streams):
        plan = plan_event(st, None, None)
        pcs = [dict(x=pc["source"].data, component=pc["component"], keep_lo=pc["keep_lo"], keep_n=pc["keep_n"], dst=pc["dst"])
               for pc in plan["pieces"]]
        L = plan["samples"]
        truth_ld, bar_new = R.assemble_truth(L, pcs)
        assert R.worst_ratio(bank.trace(i), truth_ld, bar_new) <= 1.0
        truth = truth_ld.astype(np.float64)
        e = bar_new.astype(np.float64) + _old_bar(truth, pcs, L)
        for k in range(3):
            start = int(rows["start"][3 * i + k])
            j = np.arange(start, start + Tw)
            inside = (j >= 0) & (j < L)
            w = np.where(inside, truth[:, np.clip(j, 0, L - 1)], 0.0)
            e_w = np.where(inside, e[:, np.clip(j, 0, L - 1)], 0.0).max(axis=1)
            D = np.abs(w - w.mean(axis=1, keepdims=True)).max(axis=1) + 1e-10
            has = D > 1.0  # (a row without a trace is all zeros in both banks: 0 / 1e-10 twice)
            bar_x = np.where(has, 4 * e_w / np.where(has, D - 2 * e_w, 1.0) + 2.0 ** -23 + 1e-12, 0.0)
            d = np.abs(xn[3 * i + k] - xo[3 * i + k]).max(axis=1)
            print(f"event {i} window {k}: max |x_new - x_old| = {d}, bar = {bar_x}")
            assert (d <= bar_x).all(), (i, k, d, bar_x)
            worst = max(worst, float((d[has] / bar_x[has]).max()))
    assert 0.0 <= worst <= 1.0
    bank.close()
    old.close()


def test_attributes_equal_the_host_routes():
    """Compared on integer-valued events on which both banks are bit-equal (every mean is an integer, every sum exact), so the
    same attribute kernel sees the same floats and must return the same numbers: no bar to propagate."""
    from volpick_amd import bank_attributes, bank_from_streams

    made = [make([("HHZ", 0.0, 3000), ("HHN", 0.0, 3000), ("HHE", 0.0, 3000)], seed=70 + i) for i in range(3)]
    for _, st in made:
        for tr in st:
            x = tr.data.astype(np.int64)
            x[1000:1500] *= 7  # something for the SNR to see
            x[-1] -= x.sum() % len(x)
            assert x.sum() % len(x) == 0 and np.abs(x).max() < 2 ** 23
            tr.data = x.astype(np.int32)
    streams = [st for _, st in made]
    t0 = streams[0][0].stats.starttime
    meta = {"trace_p_arrival_time": [str(t0 + 10.0), str(t0 + 9.0), None],
            "trace_s_arrival_time": [str(t0 + 15.0), None, str(t0 + 14.0)], "source_id": ["a", "b", "a"]}
    bank, table = bank_from_streams(streams, meta, attributes=True)
    arrays = [vio.stream_to_array(st.copy().detrend("demean"))[1] for st in streams]
    old = generate.WaveformBank(arrays, {"P": table["trace_p_arrival_sample"], "S": table["trace_s_arrival_sample"]})
    for i, a in enumerate(arrays):
        assert np.array_equal(bank.trace(i), a.astype(np.float32)) and np.array_equal(old.trace(i), bank.trace(i))
    want = bank_attributes(old, 100)
    for k in ("trace_snr_db", "trace_mean_snr_db", "trace_frequency_index"):
        assert np.array_equal(table[k], want[k], equal_nan=True), k
    assert np.isfinite(table["trace_frequency_index"]).all() and np.isfinite(table["trace_mean_snr_db"][:2]).all()
    fi = want["trace_frequency_index"]
    assert np.array_equal(table["source_frequency_index"], np.array([np.mean(fi[[0, 2]]), fi[1], np.mean(fi[[0, 2]])]))
    bank.close()
    old.close()
