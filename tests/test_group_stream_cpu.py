"""models._group_stream (host path) against tests/stream_restate.py: seeded irregular layouts and hand cases; at the end
the file route (io.plan_file_blocks), which asks the same planner, beside it on the same layouts.

Everything is compared for equality -- block count, trace id, start in microseconds, shape, the bits of the float32 block:
the assembly copies samples and casts each once, so there is no rounding to allow for."""
import warnings

import numpy as np
import pytest

import volpick_amd as va
import volpick_amd.io as vio
from tests import stream_restate as R
from tests.files_util import layout_bytes, planned_blocks, table_layout
from tests.files_util import trace as file_trace
from volpick_amd.models import _group_stream, _Rows, _trigger_columns

T = 301  # the issue's window length for the CPU layouts: large enough for every relation between pieces, small enough for 300
SHORT = "fragments shorter than the number of input samples"
T0 = 1_600_000_000_000_000


def to_stream(layout, rate=100.0):
    return va.Stream([va.Trace(x, dict(network=n, station=s, location=l, channel=c, starttime=va.UTCDateTime._from_us(us),
                                       sampling_rate=rate)) for n, s, l, c, us, x in layout])


def grouped(layout, in_samples=T, order="ZNE", copy=True):
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*" + SHORT)
        return list(_group_stream(to_stream(layout), order, 100.0, copy, in_samples))


def assert_blocks_equal(got, want, what=""):
    assert len(got) == len(want), f"{what}: {len(got)} blocks, the rule gives {len(want)}"
    for i, (g, (tid, us, data)) in enumerate(zip(got, want)):
        a = np.asarray(g["data"])
        assert (g["trace_id"], g["starttime"]._us) == (tid, us), f"{what}: block {i}"
        assert a.shape == data.shape and a.dtype == np.float32, f"{what}: block {i}"
        assert np.array_equal(a.view(np.uint32), data.view(np.uint32)), f"{what}: block {i} differs in " \
            f"{int((a.view(np.uint32) != data.view(np.uint32)).sum())} cells"
        assert f"{g['network']}.{g['station']}.{g['location']}" == tid


def test_random_layouts_equal_the_restated_rule():
    """300 seeded layouts.  Not vacuous: >= 90 % of them yield a block, >= 500 blocks in all; both assembly forms (the
    ``_Rows`` stack and the zero fill) occur, and ``_Rows`` is taken exactly where the block is three full-length traces."""
    n_with_block = n_blocks = n_rows = 0
    for seed in range(300):
        layout = R.random_layout(np.random.default_rng(1000 + seed), T)
        got = grouped(layout)
        assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T), f"seed {1000 + seed}")
        is_rows = [isinstance(g["data"], _Rows) for g in got]
        assert is_rows == R.full_rows(layout, "ZNE", 100, T), f"seed {1000 + seed}"
        n_with_block += bool(got)
        n_blocks += len(got)
        n_rows += sum(is_rows)
    print(f"layouts with a block {n_with_block}/300, blocks {n_blocks}, of them _Rows {n_rows}")
    assert n_with_block >= 270 and n_blocks >= 500
    assert 20 <= n_rows <= n_blocks - 200


def test_random_layouts_in_another_component_order():
    """``component_order`` moves rows and decides which letters are known: 'ENZ' and a two-component 'ZN' (E, 2 unknown)."""
    for seed in range(40):
        layout = R.random_layout(np.random.default_rng(5000 + seed), T)
        for order in ("ENZ", "ZN"):
            assert_blocks_equal(grouped(layout, order=order), R.restate(layout, order, 100, T), f"seed {5000 + seed} {order}")


def tr(channel, s0, samples, sta="AAA", jitter_us=0):
    return ("XX", sta, "", channel, T0 + 10_000 * s0 + jitter_us, samples)


def ramp(n, first=1.0, dtype=np.float32):
    return (np.arange(n) + first).astype(dtype)


def test_masked_samples_are_zero_on_both_forms():
    mask = np.zeros(400, bool)
    mask[[0, 17, 399]] = True
    masked = np.ma.masked_array(ramp(400), mask=mask)
    for layout in ([tr("HHZ", 0, masked), tr("HHN", 0, ramp(400, 1000)), tr("HHE", 0, ramp(400, 2000))],  # the stack
                   [tr("HHZ", 0, masked), tr("HHN", 5, ramp(400, 1000))]):                                # the zero fill
        got = grouped(layout)
        assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T))
        z = np.asarray(got[0]["data"])[0]
        assert (z[[0, 17, 399]] == 0).all() and z[1] == 2 and z[398] == 399
    assert isinstance(grouped([tr("HHZ", 0, masked), tr("HHN", 0, ramp(400)), tr("HHE", 0, ramp(400))])[0]["data"], _Rows)


def test_zero_length_trace_covers_nothing_but_may_set_the_origin():
    empty = np.zeros(0, np.float32)
    inside = [tr("HHZ", 0, ramp(400)), tr("HHN", 100, empty)]
    got = grouped(inside)
    assert_blocks_equal(got, R.restate(inside, "ZNE", 100, T))
    assert len(got) == 1 and got[0]["starttime"]._us == T0 and np.asarray(got[0]["data"]).shape == (3, 400)
    # the earliest trace of the instrument is the empty one: sample 0 of the instrument is ITS start, the block starts at
    # the first covered sample
    early = [tr("HHZ", 0, ramp(400)), tr("HHN", -250, empty)]
    got = grouped(early)
    assert_blocks_equal(got, R.restate(early, "ZNE", 100, T))
    assert len(got) == 1 and got[0]["starttime"]._us == T0 and np.asarray(got[0]["data"])[0, 0] == 1
    assert grouped([tr("HHZ", 0, empty)]) == []  # nothing covered: no run, no block, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert list(_group_stream(to_stream([tr("HHZ", 0, empty)]), "ZNE", 100.0, True, T)) == []


def test_a_run_of_exactly_in_samples_is_kept_and_one_shorter_is_dropped_with_the_warning():
    exact = [tr("HHZ", 0, ramp(200)), tr("HHN", 200, ramp(T - 200))]  # two abutting pieces: one run of T samples
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = list(_group_stream(to_stream(exact), "ZNE", 100.0, True, T))
    assert_blocks_equal(got, R.restate(exact, "ZNE", 100, T))
    assert len(got) == 1 and np.asarray(got[0]["data"]).shape == (3, T)
    short = [tr("HHZ", 0, ramp(200)), tr("HHN", 200, ramp(T - 201))]
    with pytest.warns(UserWarning, match=SHORT):
        got = list(_group_stream(to_stream(short), "ZNE", 100.0, True, T))
    assert got == [] == R.restate(short, "ZNE", 100, T)
    gap = [tr("HHZ", 0, ramp(200)), tr("HHN", 201, ramp(T))]  # one sample missing between them: two runs, the first too short
    with pytest.warns(UserWarning, match=SHORT):
        got = list(_group_stream(to_stream(gap), "ZNE", 100.0, True, T))
    assert_blocks_equal(got, R.restate(gap, "ZNE", 100, T))
    assert len(got) == 1 and got[0]["starttime"]._us == T0 + 2_010_000


def test_an_instrument_of_unknown_components_only_is_an_all_zero_block():
    """What the code does today, pinned: a trace whose component letter is neither in ``component_order`` nor 1/2/3 covers
    samples without writing any, so an instrument that has nothing else still yields a block -- of zeros.  (SeisBench drops
    such traces before it groups and yields nothing for the instrument; see LOG.md.)"""
    layout = [tr("HHX", 0, ramp(400)), tr("HHZ", 0, ramp(400), sta="BBB")]
    got = grouped(layout)
    assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T))
    assert [g["trace_id"] for g in got] == ["XX.AAA.", "XX.BBB."]
    a = got[0]["data"]
    assert isinstance(a, np.ndarray) and a.shape == (3, 400) and not a.any()
    # beside known components the unknown one extends the run and is otherwise invisible -- the stack form included
    layout = [tr("HHZ", 0, ramp(350)), tr("HHX", 300, ramp(200))]
    got = grouped(layout)
    assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T))
    assert got[0]["data"].shape == (3, 500) and not got[0]["data"][:, 350:].any()
    layout = [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ZNEX")]
    assert isinstance(grouped(layout)[0]["data"], _Rows)


def test_of_two_equally_long_overlapping_traces_the_later_one_wins():
    a, b = ramp(400, 1), ramp(400, 10_000)
    for first, second in ((a, b), (b, a)):
        layout = [tr("HHZ", 0, first), tr("HHZ", 100, second)]
        got = grouped(layout)
        assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T))
        z = got[0]["data"][0]
        assert np.array_equal(z[:100], first[:100]) and np.array_equal(z[100:], second)
        layout = layout[::-1]  # the same two traces, the other one later in the stream
        z = grouped(layout)[0]["data"][0]
        assert_blocks_equal(grouped(layout), R.restate(layout, "ZNE", 100, T))
        assert np.array_equal(z[:400], first) and np.array_equal(z[400:], second[300:])
    longer = [tr("HHZ", 100, ramp(401, 10_000)), tr("HHZ", 0, a)]  # one sample longer beats later
    z = grouped(longer)[0]["data"][0]
    assert_blocks_equal(grouped(longer), R.restate(longer, "ZNE", 100, T))
    assert np.array_equal(z[:100], a[:100]) and np.array_equal(z[100:], ramp(401, 10_000))


def test_aliases_and_sub_sample_starts():
    layout = [tr("HH3", 0, ramp(400, 1), jitter_us=1900), tr("HH1", 50, ramp(400, 1000), jitter_us=-1900),
              tr("HH2", 0, ramp(450, 2000))]
    got = grouped(layout)
    assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T))
    a = got[0]["data"]
    assert a.shape == (3, 450) and a[0, 0] == 1 and a[1, 50] == 1000 and a[1, 49] == 0 and a[2, 0] == 2000
    # where 'Z' and '3' both exist they are the same component: the longer one wins the overlap
    layout = [tr("HHZ", 0, ramp(400, 1)), tr("HH3", 0, ramp(350, 5000))]
    assert_blocks_equal(grouped(layout), R.restate(layout, "ZNE", 100, T))
    assert grouped(layout)[0]["data"][0, 0] == 1


def test_int32_counts_beyond_2_24_are_rounded_once():
    counts = np.array([2**24 + 1, 2**24 + 3, -(2**30) - 65, 2**31 - 1] * 100, np.int32)
    f64 = np.array([1 / 3, 16777217.0, 1e-50, -2.5e-46] * 100)
    layout = [tr("HHZ", 0, counts), tr("HHN", 0, f64), tr("HHE", 0, ramp(400))]
    got = grouped(layout)
    assert isinstance(got[0]["data"], _Rows)
    assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T))
    assert np.array_equal(np.asarray(got[0]["data"])[0], counts.astype(np.float32))
    ragged = layout[:2] + [tr("HHE", 1, ramp(400))]
    assert_blocks_equal(grouped(ragged), R.restate(ragged, "ZNE", 100, T))


def test_copy_true_leaves_every_input_array_and_header_untouched():
    rng = np.random.default_rng(77)
    layout = R.random_layout(rng, T) + R.random_layout(rng, T)
    mask = rng.random(500) < 0.1
    layout.append(tr("HHZ", 0, np.ma.masked_array(ramp(500), mask=mask), sta="MSK"))
    st = to_stream(layout)
    st.append(va.Trace(rng.standard_normal(400), dict(network="XX", station="SLOW", channel="HHZ", sampling_rate=50.0,
                                                      starttime=va.UTCDateTime._from_us(T0))))  # resampled -- on a copy
    arrays = [t.data for t in st]
    before = [(np.ma.getdata(a).tobytes(), np.ma.getmaskarray(a).tobytes(), a.dtype, dict(t.stats)) for a, t in zip(arrays, st)]
    traces = list(st)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*" + SHORT)
        blocks = list(_group_stream(st, "ZNE", 100.0, True, T))
        for g in blocks:
            np.asarray(g["data"])
    assert len(blocks) >= 4 and any(g["station"] == "SLOW" for g in blocks)
    assert list(st) == traces
    for a, t, (data, mask_, dtype, stats) in zip(arrays, st, before):
        assert t.data is a and a.dtype == dtype and dict(t.stats) == stats
        assert np.ma.getdata(a).tobytes() == data and np.ma.getmaskarray(a).tobytes() == mask_


class SlotModel:
    """Stands in for the model under ``_ClassifyRun`` and keeps the library's two rules about submit slots: a slot holds one
    uncollected submit (vp_classify_submit), and the multi-block call wants every slot of context 0 free (vp_classify_multi)."""

    in_samples, n_contexts, _timing, _seg_per_context = T, 3, None, 2

    def __init__(self, max_windows):
        self._max_windows_per_call, self.busy, self.calls = max_windows, set(), []

    def _submit_block(self, ctx, data, args, specs, cap):
        assert (ctx, 0) not in self.busy, f"slot 0 of context {ctx} has an uncollected submit"
        self.busy.add((ctx, 0))
        self.calls.append(("submit", ctx))
        return {"ctx": ctx}

    def _collect_block(self, job, args, specs, columns=False):
        self.busy.remove((job["ctx"], 0))
        return _trigger_columns([(0, 1, 2, 1, 0.5)]), 1

    def _classify_blocks(self, groups, args, specs, columns=False):
        assert not any(ctx == 0 for ctx, _ in self.busy), "uncollected vp_classify_submit on this handle"
        self.calls.append(("multi", len(groups)))
        return [_trigger_columns([(0, 1, 2, 1, 0.5)]) for _ in groups]


@pytest.mark.parametrize("max_windows,flushed", [(8, ("multi", 2)), (4, ("submit", 0))])
def test_a_resident_chunk_that_fills_up_while_the_host_ring_is_busy(max_windows, flushed):
    """Found by tests/test_gpu_stream_layouts.py: a chunk of device-resident blocks that reached ``_max_windows_per_call`` in
    MID-stream was sent while a host block was still uncollected on context 0, whose slots it needs -- the library refused
    the call.  (At the end of a call the host route was always drained first.)"""
    from volpick_amd.models import _ClassifyRun

    model = SlotModel(max_windows)
    run = _ClassifyRun(model, {"overlap": 0}, [(1, "P", 0.3, 0.3)])
    block = lambda sta, n: dict(data=np.zeros((3, n), np.float32), trace_id=sta, starttime=va.UTCDateTime(0))  # noqa: E731
    run.add_host(block("H0", 2 * T))
    for k in range(3):
        run.add_resident(block(f"R{k}", 3 * T))  # 4 windows each, by the run's own count
    assert model.calls[0] == ("submit", 0) and model.calls.count(flushed) == (3 if flushed == ("submit", 0) else 1)
    run.drain_long(), run.drain_host(), run.drain_resident()
    assert not model.busy and sorted(run.tids) == ["H0", "R0", "R1", "R2"] and run.tids[0] == "H0"


@pytest.mark.parametrize("name,layout,rows", [
    ("three full traces", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ENZ")], True),
    ("three full traces, aliased", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("Z12")], True),
    ("mixed dtypes", [tr("HHZ", 0, ramp(350, 1, np.int32)), tr("HHN", 0, ramp(350, 2, np.float64)), tr("HHE", 0, ramp(350))], True),
    ("starts 0.2 sample apart", [tr("HHZ", 0, ramp(350), jitter_us=2000), tr("HHN", 0, ramp(350)), tr("HHE", 0, ramp(350))], True),
    ("an empty fourth trace", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ZNE")] + [tr("HHZ", 10, np.zeros(0))], True),
    ("one trace a sample short", [tr("HHZ", 0, ramp(350)), tr("HHN", 0, ramp(350)), tr("HHE", 0, ramp(349))], False),
    ("one trace a sample late", [tr("HHZ", 0, ramp(350)), tr("HHN", 0, ramp(350)), tr("HHE", 1, ramp(349))], False),
    ("two components", [tr("HHZ", 0, ramp(350)), tr("HHN", 0, ramp(350))], False),
    ("a second full Z", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ZNEZ")], False),
    ("Z and its alias 3", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ZN3")], False),
    ("a fragment inside a full component", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ZNE")] + [tr("HHE", 7, ramp(5))], False),
    ("a piece that abuts: the run is longer than the traces", [tr("HH" + c, 0, ramp(350, k)) for k, c in enumerate("ZNE")] + [tr("HHZ", 350, ramp(9))], False),
])
def test_the_rows_form_is_taken_exactly_for_three_full_length_traces(name, layout, rows):
    got = grouped(layout)
    assert len(got) == 1 and isinstance(got[0]["data"], _Rows) == rows == R.full_rows(layout, "ZNE", 100, T)[0]
    assert_blocks_equal(got, R.restate(layout, "ZNE", 100, T), name)
    assert_blocks_equal(grouped(layout[::-1]), R.restate(layout[::-1], "ZNE", 100, T), name + ", reversed")


# --------------------------------------------------------------------------- one planner, two callers
# ``_group_stream`` and the file route (``io.scan_segments`` + ``io.plan_file_blocks``) ask ``stream.plan_blocks`` which samples
# form a block.  Before they shared it each worded these relations in its own way: held here, through both, against the rule.
def n(channel, samples, first=0):
    return file_trace(channel, samples, first, np.random.default_rng(samples + first))


@pytest.mark.parametrize("name,traces,order,shapes,short", [
    ("a piece that ends exactly at the run's end", [n("HHZ", 500), n("HHN", 300, 200)], "ZNE", [(3, 500)], 0),
    ("a piece that starts exactly at the end of the run so far: it merges", [n("HHZ", 400), n("HHN", 350, 400)], "ZNE", [(3, 750)], 0),
    ("a piece one sample past the run's end: a new run", [n("HHZ", 400), n("HHN", 350, 401)], "ZNE", [(3, 400), (3, 350)], 0),
    ("... which is too short", [n("HHZ", 400), n("HHN", 300, 401)], "ZNE", [(3, 400)], 1),
    ("an unknown component bridges two known ones", [n("HHZ", 350), n("HHX", 100, 350), n("HHN", 350, 450)], "ZNE", [(3, 800)], 0),
    ("... and without it they are two runs", [n("HHZ", 350), n("HHN", 350, 450)], "ZNE", [(3, 350), (3, 350)], 0),
    ("1 / 2 / 3 are N / E / Z", [n("HH3", 400), n("HH1", 350, 50), n("HH2", 450)], "ZNE", [(3, 450)], 0),
    ("2 is E, which 'ZN' has no row for: it still extends the run", [n("HH3", 400), n("HH1", 350, 50), n("HH2", 450)], "ZN", [(2, 450)], 0),
])
def test_both_callers_of_the_planner_equal_the_restated_rule(lib, name, traces, order, shapes, short):
    table, seg = vio.scan_segments(layout_bytes(traces))
    layout = table_layout(table, seg)  # samples: 1 + their number in the file
    want = R.restate(layout, order, 100, T)
    assert [data.shape for _, _, data in want] == shapes and R.short_runs(layout, order, 100, T) == short, name
    with warnings.catch_warnings(record=True) as warned:
        warnings.simplefilter("always")
        got = list(_group_stream(to_stream(layout), order, 100.0, True, T))
    assert_blocks_equal(got, want, name + ", assembly")
    assert len(warned) == short and all(SHORT in str(w.message) for w in warned)
    with warnings.catch_warnings(record=True) as warned:
        warnings.simplefilter("always")
        plan = vio.plan_file_blocks(table, seg, order, 100.0, T)
    assert plan.reason is None and plan.short_runs == len(warned) == short and all(SHORT in str(w.message) for w in warned)
    cells = planned_blocks(table, plan)
    assert len(cells) == len(want), name
    for b, c, (trace_id, start_us, data) in zip(plan.blocks, cells, want):
        assert (b["trace_id"], b["start_us"], b["shape"]) == (trace_id, start_us, data.shape), name + ", file route"
        assert np.array_equal(c, data), name + ", file route"
