"""GPU: irregular streams through the assembly on the device and through the three classify routes.

The expected value of every test is built from tests/stream_restate.py: the blocks the assembly rule gives, each taken ALONE
through ``_classify_block`` / ``_annotate_data``, times built here as block start + rint(k / rate * 1e6) microseconds.  All
comparisons are for equality: the assembly copies samples (each cast to float32 once) and tests/test_gpu_async.py
establishes that the routes are bit-identical on regular layouts.  Only the oracle comparison has a tolerance: the bar of
tests/test_gpu_phasenet.py:204-215 and tests/test_gpu_eqt.py:325-336 (offset and length equal, NaN pattern equal, max
|hip - oracle| < 1e-4)."""
import numpy as np
import pytest
import torch

import volpick_amd as va
from tests import stream_restate as R
from volpick_amd import models as M
from volpick_amd.synthetic import synthetic_stream_array

pytestmark = pytest.mark.gpu

RATE = 100
TOL = 1e-4  # tests/test_gpu_phasenet.py:14, tests/test_gpu_eqt.py:14
T0 = 1_600_000_000_000_000
KW = dict(P_threshold=0.2, S_threshold=0.2)


def to_stream(layout):
    return va.Stream([va.Trace(x, dict(network=n, station=s, location=l, channel=c, starttime=va.UTCDateTime._from_us(us),
                                       sampling_rate=float(RATE))) for n, s, l, c, us, x in layout])


def moved(stream, which=None):
    """The stream with the traces ``which`` (indices; None: all) device-backed, the order kept."""
    out = list(stream)
    idx = range(len(out)) if which is None else which
    for i, tr in zip(idx, va.to_device(va.Stream([out[i] for i in idx]))):
        out[i] = tr
    return va.Stream(out)


def grouped(stream, in_samples):
    import warnings

    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*fragments shorter")
        return list(M._group_stream(stream, "ZNE", float(RATE), True, in_samples))


def host_bits(data):
    a = data.cpu().numpy() if torch.is_tensor(data) else np.asarray(data)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def assert_blocks_equal(got, want, what):
    assert len(got) == len(want), what
    for i, (g, (tid, us, data)) in enumerate(zip(got, want)):
        assert (g["trace_id"], g["starttime"]._us, tuple(g["data"].shape)) == (tid, us, data.shape), f"{what}: block {i}"
        assert np.array_equal(host_bits(g["data"]), data.view(np.uint32)), f"{what}: block {i}"


# --------------------------------------------------------------------------- a. assembly on the device
def full_mixed(sta, n, first=0):
    """Three full-length traces of three dtypes, counts beyond 2^24 among them: the device stack with promotion."""
    rng = np.random.default_rng(n)
    return [("XX", sta, "", "HHZ", T0 + 10_000 * first, rng.integers(-2**30, 2**30, n).astype(np.int32)),
            ("XX", sta, "", "HH1", T0 + 10_000 * first + 1500, rng.standard_normal(n) * 1e3),
            ("XX", sta, "", "HH2", T0 + 10_000 * first - 1500, (rng.standard_normal(n) * 1e3).astype(np.float32))]


def test_device_assembly_equals_the_restated_rule_bit_for_bit():
    """40 seeded layouts at PhaseNet's window length, every trace device-backed, dtypes mixed inside instruments.  Not
    vacuous: both device forms occur (the stack of three full traces, of mixed dtypes too, and the zero fill)."""
    T = va.PhaseNet.in_samples
    n_blocks = n_stack = n_stack_mixed = 0
    for seed in range(40):
        layout = R.random_layout(np.random.default_rng(2000 + seed), T)
        if seed % 8 == 0:
            layout += full_mixed("ZZ9", T + 7 + seed)
        st = moved(to_stream(layout))
        assert all(tr._dev is not None and tr._dev.is_cuda for tr in st)
        got = grouped(st, T)
        want = R.restate(layout, "ZNE", RATE, T)
        assert_blocks_equal(got, want, f"seed {2000 + seed}")
        for g, (_, _, data) in zip(got, want):  # on the device -- but for a block that only an unknown component covers: zeros
            assert (torch.is_tensor(g["data"]) and g["data"].is_cuda and g["data"].dtype == torch.float32) or not data.any()
        full = R.full_rows(layout, "ZNE", RATE, T)
        n_blocks += len(got)
        n_stack += sum(full)
        n_stack_mixed += sum(f and g["station"] == "ZZ9" for f, g in zip(full, got))
        assert all(tr._data is None for tr in st), "the device assembly read a host copy"
    print(f"device layouts: {n_blocks} blocks, {n_stack} of them one stack ({n_stack_mixed} of mixed dtypes)")
    assert n_blocks >= 60 and n_stack >= 8 and n_stack_mixed == 5 and n_blocks - n_stack >= 30


def test_a_stream_partly_on_the_device_gives_the_host_result():
    """Some traces on the host, some on the device: instruments wholly on the device are assembled there, the others on the
    host from downloaded copies; either way the rule's bits."""
    T = va.PhaseNet.in_samples
    kinds = set()
    for seed in range(10):
        rng = np.random.default_rng(3000 + seed)
        layout = R.random_layout(rng, T)
        layout += full_mixed("ZZ8", T + 3) + full_mixed("ZZ6", T + 5)[:2] + [
            ("XX", "ZZ7", "", "HHZ", T0, np.arange(T + 40, dtype=np.float64)),
            ("XX", "ZZ7", "", "HHN", T0 + 200_000, np.arange(T, dtype=np.int32))]
        host = to_stream(layout)
        sta = [l[1] for l in layout]
        which = [i for i in range(len(layout)) if rng.random() < 0.5 and sta[i] not in ("ZZ6", "ZZ7", "ZZ8")]
        which += [i for i in range(len(layout)) if (sta[i], layout[i][3]) in (("ZZ8", "HHZ"), ("ZZ8", "HH2"), ("ZZ7", "HHN"))]
        which += [i for i in range(len(layout)) if sta[i] == "ZZ6"]  # wholly on the device: assembled there
        st = moved(host, sorted(which))
        got = grouped(st, T)
        assert_blocks_equal(got, R.restate(layout, "ZNE", RATE, T), f"seed {3000 + seed}")
        assert_blocks_equal(grouped(host, T), R.restate(layout, "ZNE", RATE, T), f"seed {3000 + seed} (host)")
        by_sta = {g["station"]: type(g["data"]).__name__ for g in got}
        assert by_sta["ZZ8"] == "_Rows" and by_sta["ZZ7"] == "ndarray" and by_sta["ZZ6"] == "Tensor"  # mixed backing: the host forms
        kinds |= {type(g["data"]).__name__ for g in got}
    assert kinds == {"Tensor", "_Rows", "ndarray"}


# --------------------------------------------------------------------------- the streams of b, c, d: synthetic events
def station(sta, data, first, pieces, loc=""):
    """Traces cut from a (3, n) ZNE array: ``pieces`` is [(channel letter, row, s0, s1, gain, dtype)], a piece the samples
    [s0, s1) of ``row`` times ``gain`` (a rival piece with another gain makes the overlap winner visible), starting at
    sample ``first + s0`` of the call's clock, 1.3 ms off the grid."""
    out = []
    for letter, row, s0, s1, gain, dtype in pieces:
        x = data[row, s0:s1].astype(np.float64) * gain
        x = np.rint(x * 1e5).astype(np.int32) if dtype is np.int32 else x.astype(dtype)
        out.append(("XX", sta, loc, "HH" + letter, T0 + 10_000 * (first + s0) + 1300, x))
    return out


def regular(n, dtypes=(np.float32,) * 3, letters="ZNE"):
    return [(letters[c], c, 0, n, 1.0, dtypes[c]) for c in range(3)]


def ragged(n, variant):
    """Irregular pieces over [0, n): late / early components, an overlap with a rival, aliases, a missing component."""
    f32, f64, i32 = np.float32, np.float64, np.int32
    return [
        [("Z", 0, 0, n, 1.0, f32), ("N", 1, 250, n, 1.0, f64), ("E", 2, 0, n - 333, 1.0, i32)],
        [("3", 0, 0, n // 2 + 100, 1.0, f32), ("3", 0, n // 2, n, 0.5, f32), ("1", 1, 0, n, 1.0, f32), ("2", 2, 17, n, 1.0, f64)],
        [("Z", 0, 0, n, 1.0, i32), ("N", 1, 0, n, 1.0, f32)],
        [("Z", 0, 0, n - 300, 1.0, f32), ("Z", 0, 100, n, 3.0, f32), ("N", 1, 0, n, 1.0, f32), ("E", 2, 0, n, 1.0, f32),
         ("X", 2, 0, n, 1.0, f32)],
        [("Z", 0, 5, n, 1.0, f64), ("N", 1, 0, n // 3, 1.0, f32), ("N", 1, n // 3, n, 1.0, i32), ("E", 2, 0, n, 1.0, f32)],
    ][variant % 5]


def events(n):
    return max(2, n // 2500)


def route_stream(m, args):
    """(layout, device-backed station names, name of the station a gap splits) for one classify() call through all routes."""
    T, step, nc = m.in_samples, m.in_samples - args["overlap"], m.n_contexts
    n_long = T + (4 * nc - 1) * step + 37  # batch_size 2: long from 2 * batch * contexts windows on
    assert m._is_long(n_long - 37, args) and not m._is_long(n_long - 38, args)
    roles = list("HRLHRHLRHRH") + ["H"] * (nc + 2 - 5)  # sorted station order: the routes interleave
    assert roles.count("H") == nc + 2 and roles.count("R") == 4 and roles.count("L") == 2
    # the run counts one window more per block (the tail): 4, 3, 7, 6 -- at 8 windows per call the chunks are [4 + 3], [7], [6]
    resident_windows = iter([3, 2, 6, 5])
    layout, on_device, k_host, k_long, gap = [], [], 0, 0, None
    for k, role in enumerate(roles):
        sta, first = f"S{k:02d}", 700 * k
        if role == "L":
            n = n_long + 11 * k_long
            data, _, _ = synthetic_stream_array(n, seed=8000 + k, n_events=events(n))
            layout += station(sta, data, first, regular(n) if k_long == 0 else ragged(n, 0))
            on_device += [sta] * (k_long == 1)  # the second long block is cut from a device array
            k_long += 1
        elif role == "R":
            n = T + (next(resident_windows) - 1) * step + 13 * k
            data, _, _ = synthetic_stream_array(n, seed=8000 + k, n_events=events(n))
            layout += station(sta, data, first, regular(n, (np.int32, np.float64, np.float32), "Z12") if k == 1 else ragged(n, k))
            on_device.append(sta)
        elif k_host == 1:  # a gap of 5 s splits this station into two blocks of one trace id
            n1, n2 = T + step + 21, T + 2 * step + 5
            data, _, _ = synthetic_stream_array(n1 + 500 + n2, seed=8000 + k, n_events=events(n1 + n2) + 2)
            layout += station(sta, data, first, [(c, i, 0, n1, 1.0, np.float32) for i, c in enumerate("ZNE")] +
                              [(c, i, n1 + 500, n1 + 500 + n2, 1.0, np.float32) for i, c in enumerate("ZNE")])
            gap, k_host = sta, k_host + 1
        else:
            n = T + (1 + k_host % 3) * step + 29 * k
            data, _, _ = synthetic_stream_array(n, seed=8000 + k, n_events=events(n))
            layout += station(sta, data, first, regular(n) if k_host == 0 else ragged(n, k_host))
            k_host += 1
    order = np.random.default_rng(5).permutation(len(layout))
    return [layout[i] for i in order], on_device, gap


def as_stream(layout, on_device):
    return moved(to_stream(layout), [i for i, l in enumerate(layout) if l[1] in on_device])


def expected_records(m, layout, args):
    """Every restated block alone through ``_classify_block`` -> (picks, detections) as sorted tuples in microseconds."""
    specs = m._trigger_specs(args)
    picks, dets = [], []
    us = lambda t0, k: t0 + int(np.rint(k / float(RATE) * 1e6))  # noqa: E731
    for tid, t0, data in R.restate(layout, m.component_order, RATE, m.in_samples):
        for spec, on, off, peak, value in m._classify_block(data, args, specs)[0]:
            label = specs[spec][1]
            if label == "Detection":
                dets.append((us(t0, on), tid, us(t0, off), value))
            else:
                picks.append((us(t0, on), tid, label, us(t0, off), us(t0, peak), value))
    return sorted(picks, key=lambda p: p[:3]), sorted(dets, key=lambda d: d[:2])


def got_records(out):
    return ([(p.start_time._us, p.trace_id, p.phase, p.end_time._us, p.peak_time._us, p.peak_value) for p in out.picks],
            [(d.start_time._us, d.trace_id, d.end_time._us, d.peak_value) for d in out.detections])


@pytest.fixture(scope="module", params=[va.PhaseNet, va.EQTransformer], ids=["phasenet", "eqtransformer"])
def routed(request):
    m = request.param.from_pretrained("volpick").cuda()
    kw = dict(KW, batch_size=2)
    args = m._argdict(kw)
    assert args["overlap"] == {"PhaseNet": 1500, "EQTransformer": 1800}[m.name]
    layout, on_device, gap = route_stream(m, args)
    return dict(m=m, kw=kw, layout=layout, on_device=on_device, gap=gap, want=expected_records(m, layout, args))


@pytest.fixture
def spy(monkeypatch):
    """Counts what a classify() call enters: the route of every block, the size of every resident chunk, the submit slots
    of the long route and the contexts of the host ring."""
    seen = dict(routes=[], chunks=[], slot_bases=[], contexts=[])
    run = M._ClassifyRun
    for route in ("long", "resident", "host"):
        inner = getattr(run, "add_" + route)
        monkeypatch.setattr(run, "add_" + route, lambda self, grp, inner=inner, route=route: (seen["routes"].append(route), inner(self, grp))[1])
    drain = run.drain_resident
    monkeypatch.setattr(run, "drain_resident", lambda self: (seen["chunks"].append(len(self.chunk)) if self.chunk else None, drain(self))[1])
    submit, block = M.WaveformModel._segments_submit, M.WaveformModel._submit_block
    monkeypatch.setattr(M.WaveformModel, "_segments_submit",
                        lambda self, data, args, slot_base, *a: (seen["slot_bases"].append(slot_base), submit(self, data, args, slot_base, *a))[1])
    monkeypatch.setattr(M.WaveformModel, "_submit_block",  # (a resident chunk of one block goes this way too, on context 0)
                        lambda self, ctx, *a: (seen["contexts"].append((seen["routes"][-1], ctx)), block(self, ctx, *a))[1])
    return seen


@pytest.mark.parametrize("variant", ["one chunk", "three chunks", "not batched across blocks"])
def test_one_classify_call_through_all_three_routes(routed, spy, monkeypatch, variant):
    """Long, host and resident blocks interleaved in one call, the host ring wrapping, two long blocks (both sets of submit
    slots): the picks are those of every block alone, times from the block's own start."""
    m, nc = routed["m"], routed["m"].n_contexts
    if variant == "three chunks":
        monkeypatch.setattr(m, "_max_windows_per_call", 8)
    if variant == "not batched across blocks":
        monkeypatch.setattr(m, "batch_across_blocks", False)
    got = got_records(m.classify(as_stream(routed["layout"], routed["on_device"]), **routed["kw"]))
    want = routed["want"]
    print(f"{m.name}, {variant}: {len(want[0])} picks, {len(want[1])} detections; routes {spy['routes']}, resident chunks "
          f"{spy['chunks']}, long slot bases {spy['slot_bases']}, short contexts {spy['contexts']}")
    assert len(want[0]) >= 30
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])
    for a, b in zip(got[0] + got[1], want[0] + want[1]):
        assert a == b
    routes = spy["routes"]
    changes = sum(a != b for a, b in zip(routes, routes[1:]))
    assert routes.count("long") == 2 and spy["slot_bases"] == [0, m._seg_per_context]  # both sets of submit slots
    if variant == "not batched across blocks":
        assert routes.count("resident") == 0 and routes.count("host") == nc + 3 + 4
    else:
        assert routes.count("resident") == 4 and routes.count("host") == nc + 3  # (the split station: two blocks)
        assert changes >= 8  # the routes interleave
        assert spy["chunks"] == ([4] if variant == "one chunk" else [2, 1, 1])
    ring = [ctx for route, ctx in spy["contexts"] if route == "host"]  # submitted from inside add_host
    assert ring[:nc + 1] == list(range(nc)) + [0]  # the ring wraps


def test_picks_of_a_station_split_by_a_gap(routed):
    """Both blocks carry one trace id; their picks carry their own block's start and other stations' picks sort between."""
    m, sta = routed["m"], routed["gap"]
    tid = f"XX.{sta}."
    starts = [us for t, us, _ in R.restate(routed["layout"], m.component_order, RATE, m.in_samples) if t == tid]
    assert len(starts) == 2
    picks = got_records(m.classify(as_stream(routed["layout"], routed["on_device"]), **routed["kw"]))[0]
    assert picks == routed["want"][0]
    assert picks == sorted(picks, key=lambda p: p[:3])
    mine = [i for i, p in enumerate(picks) if p[1] == tid]
    first = [i for i in mine if picks[i][0] < starts[1]]
    second = [i for i in mine if picks[i][0] >= starts[1]]
    assert first and second and max(first) < min(second)
    assert all(starts[0] <= picks[i][0] and picks[i][3] < starts[1] for i in first)  # inside their own block
    assert any(picks[i][1] != tid for i in range(max(first), min(second)))  # other stations' picks in between
    for backing in ([], [sta]):  # the two blocks alone: on the host ring, and as one resident chunk
        layout = [l for l in routed["layout"] if l[1] == sta]
        alone = got_records(m.classify(as_stream(layout, backing), **routed["kw"]))[0]
        assert alone == [p for p in picks if p[1] == tid]


# --------------------------------------------------------------------------- c. annotate
def annotate_layouts(m):
    """Ten irregular layouts at the model's window length: eight seeded ones (values: noise and counts) and two built from
    synthetic events, the first of which a gap splits."""
    T = m.in_samples
    out = [R.random_layout(np.random.default_rng(4000 + s), T) for s in range(8)]
    n1, n2 = T + 400, 2 * T + 90
    data, _, _ = synthetic_stream_array(n1 + 700 + n2, seed=4100, n_events=6)
    out.append(station("GAP", data, 0, [("Z", 0, 0, n1, 1.0, np.float32), ("N", 1, 30, n1, 1.0, np.float64),
                                        ("Z", 0, n1 + 700, n1 + 700 + n2, 1.0, np.int32), ("E", 2, n1 + 900, n1 + 700 + n2, 1.0, np.float32)]))
    data, _, _ = synthetic_stream_array(2 * T + 321, seed=4101, n_events=4)
    out.append(station("AAA", data, 50, ragged(2 * T + 321, 1)) + station("BBB", data[:, :T + 99], 10, ragged(T + 99, 4), loc="00"))
    return out


def expected_annotations(m, layout, args):
    """[(trace id, start in microseconds, samples)] from the restated blocks, each alone through ``_annotate_data``."""
    want = []
    for tid, t0, data in R.restate(layout, m.component_order, RATE, m.in_samples):
        out, fv, lv, nw = m._annotate_data(data, args)
        if nw == 0 or fv < 0:
            continue
        out = out.cpu().numpy()
        for i, label in enumerate(m.labels):
            want.append((f"{tid}.{type(m).__name__}_{label}", t0 + int(np.rint(fv / float(RATE) * 1e6)), out[i, fv:lv + 1], fv, data))
    return want


@pytest.fixture(scope="module", params=[va.PhaseNet, va.EQTransformer], ids=["phasenet", "eqtransformer"])
def annotated(request):
    m = request.param.from_pretrained("volpick").cuda()
    return m, annotate_layouts(m)


@pytest.mark.filterwarnings("ignore:Parts of the input stream consist of fragments shorter")
@pytest.mark.parametrize("backing", ["host", "device"])
def test_annotate_on_irregular_layouts(annotated, backing):
    """Trace ids, start (block start + first valid sample) and length from the restated blocks, the samples bit for bit those
    of the block alone; a gap splits one station into two blocks of one id."""
    m, layouts = annotated
    args = m._argdict({})
    n_traces, split = 0, False
    for k, layout in enumerate(layouts):
        st = to_stream(layout)
        got = m.annotate(moved(st) if backing == "device" else st)
        want = expected_annotations(m, layout, args)
        assert [tr.id for tr in got] == [w[0] for w in want], f"layout {k}"
        for tr, (_, us, samples, _, _) in zip(got, want):
            assert (tr.stats.starttime._us, tr.stats.npts, tr.stats.sampling_rate) == (us, len(samples), float(RATE)), f"layout {k}"
            assert tr.data.dtype == np.float32 and np.array_equal(tr.data.view(np.uint32), samples.view(np.uint32)), f"layout {k}"
        n_traces += len(got)
        ids = [w[0] for w in want]
        split |= any(ids.count(i) > 1 for i in ids)
    print(f"{m.name}, {backing}: {n_traces} annotation traces")
    assert n_traces >= 3 * 12 and split


def test_annotate_on_irregular_layouts_against_the_oracle(annotated):
    """The layouts of synthetic events (PhaseNet: four, EQTransformer: two; the torch-CPU oracle is slow) against
    oracle.pipeline.annotate_array on the restated block, at the bar of the stacked-annotate parity tests
    (tests/test_gpu_phasenet.py:204-215, tests/test_gpu_eqt.py:325-336)."""
    from oracle import pipeline as OP
    from oracle.models import load_pretrained

    m, layouts = annotated
    oracle = load_pretrained(m.name.lower())
    layouts = layouts[8:]
    if m.name == "PhaseNet":
        T = m.in_samples
        data, _, _ = synthetic_stream_array(3 * T, seed=4102, n_events=5)
        layouts = layouts + [station("CCC", data, 3, ragged(3 * T, 3)), station("DDD", data, 0, ragged(2 * T + 1, 2))]
    args = m._argdict({})
    assert len(layouts) == (4 if m.name == "PhaseNet" else 2)
    worst = 0.0
    for layout in layouts:
        got = m.annotate(to_stream(layout))
        blocks = R.restate(layout, m.component_order, RATE, m.in_samples)
        assert len(got) == len(m.labels) * len(blocks) > 0
        for b, (tid, t0, data) in enumerate(blocks):
            want = OP.annotate_array(oracle, data, overlap=args["overlap"], blinding=args["blinding"], stacking=args["stacking"])
            for i, (label, off, ref) in enumerate(want):
                tr = got[b * len(m.labels) + i]
                assert tr.id == f"{tid}.{type(m).__name__}_{label}"
                assert tr.stats.starttime._us == t0 + int(np.rint(off / float(RATE) * 1e6)) and tr.stats.npts == len(ref)
                assert np.array_equal(np.isnan(tr.data), np.isnan(ref))
                worst = max(worst, float(np.nanmax(np.abs(tr.data - ref))))
    print(f"{m.name}: max |hip - oracle| over {len(layouts)} layouts {worst:.2e}")
    assert worst < TOL
