"""Host side of ``classify_files`` (no GPU): the library's ordered record table (``vp_mseed_scan_segments``) against
``scan_mseed`` + ``_segments``, and the block plan from headers (``io.plan_file_blocks``) against the independent restatement
of the assembly rule (tests/stream_restate.py) and against ``models._group_stream``, both run on traces whose samples are
their own global sample numbers, so that every block cell names the record and the offset it came from."""
import ctypes as C
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

import volpick_amd.io as vio
from oracle import mseed as OM
from tests import stream_restate as R
from tests.files_util import PERIOD_US, layout_bytes, layouts, log_channel_bytes, planned_blocks, table_layout, trace
from tests.mseed_util import T0, file_bytes, mixed_file_bytes, seismogram
from volpick_amd import Stream, Trace, UTCDateTime, _lib
from volpick_amd.models import _group_stream

ROOT = Path(__file__).resolve().parents[1]
RNG = lambda seed=0: np.random.default_rng(seed)  # noqa: E731


# ------------------------------------------------------------------------------------------ vp_mseed_scan_segments
def assert_same_table(buf):
    want, want_seg = vio._segments(vio.scan_mseed(buf))
    got, got_seg = vio.scan_segments(buf)
    assert len(got) == len(want)
    for name in vio._REC_DTYPE.names:
        assert np.array_equal(got[name], want[name]), name
    assert got_seg.dtype == want_seg.dtype and np.array_equal(got_seg, want_seg)
    return got, got_seg


def records(buf, reclen=512):
    return [buf[i:i + reclen] for i in range(0, len(buf), reclen)]


def test_records_out_of_order(lib):
    rng = RNG(1)
    buf = file_bytes([trace(c, 4000, rng=rng) for c in ("HHZ", "HHN")] + [trace("HHZ", 900, 4000, rng, sta="AB")])
    recs = records(buf)
    for order in (recs[::-1], [recs[i] for i in RNG(2).permutation(len(recs))]):
        got, seg = assert_same_table(b"".join(order))
        assert seg[-1] == 2  # back in order every trace is one segment again


def test_equal_start_times_go_by_offset(lib):
    rng = RNG(3)
    one = file_bytes([trace("HHZ", 1500, rng=rng)])
    got, seg = assert_same_table(one + one + one)
    assert len(set(got["start_us"])) * 3 == len(got) and (np.diff(got["offset"].reshape(-1, 3), axis=1) > 0).all()


def test_zero_sample_record_is_dropped(lib):
    buf = bytearray(file_bytes([trace("HHZ", 3000, rng=RNG(4))]))
    buf[512 + 30:512 + 32] = b"\0\0"  # second record: no samples
    got, seg = assert_same_table(bytes(buf))
    assert len(got) == len(buf) // 512 - 1 and 512 not in got["offset"] and seg[-1] == 1


def test_int_then_float_of_one_id(lib):
    rng = RNG(5)
    a = file_bytes([trace("HHZ", 1000, rng=rng)])
    b = file_bytes([trace("HHZ", 1000, 1000, data=seismogram(1000, rng).astype(np.float32))], encoding=OM.ENC_FLOAT32)
    c = file_bytes([trace("HHZ", 1000, 2000, data=seismogram(1000, rng).astype(np.float64))], encoding=OM.ENC_FLOAT64)
    got, seg = assert_same_table(a + b + c)
    assert seg[-1] == 1  # the two float encodings are one kind


def test_rate_change(lib):
    rng = RNG(6)
    got, seg = assert_same_table(file_bytes([trace("HHZ", 1000, rng=rng), trace("HHZ", 500, 1000, rng, rate=50.0)]))
    assert seg[-1] == 1


@pytest.mark.parametrize("shift_us, chained", [(PERIOD_US // 2, True), (PERIOD_US // 2 + 1, False), (-PERIOD_US // 2, True),
                                               (-PERIOD_US // 2 - 1, False), (0, True)])
def test_next_start_at_half_a_period(lib, shift_us, chained):
    rng = RNG(7)
    a = trace("HHZ", 800, rng=rng)
    b = trace("HHZ", 800, 800, rng, shift_us=shift_us)
    got, seg = assert_same_table(file_bytes([a, b], with_b1001=True))
    assert seg[-1] == (0 if chained else 1)


def test_mixed_versions_and_record_lengths(lib):
    assert_same_table(mixed_file_bytes(n=6000))
    rng = RNG(8)
    parts = [file_bytes([trace(c, 2500, rng=rng)], reclen=reclen) for c, reclen in (("HHZ", 256), ("HHN", 512), ("HHE", 4096))]
    got, seg = assert_same_table(b"".join(parts))
    assert set(got["reclen"]) == {256, 512, 4096} and seg[-1] == 2
    for reclen in (256, 512, 4096):
        assert_same_table(file_bytes([trace(c, 2500, rng=rng) for c in "ZNE"], reclen=reclen))


def test_empty_buffer(lib):
    got, seg = assert_same_table(b"")
    assert len(got) == 0 and len(seg) == 0


def scanner_error_cases():
    rng = RNG(9)
    v3 = OM.write_mseed3([trace("HHZ", 1200, rng=rng)])
    crc = bytearray(v3)
    crc[60] ^= 1
    no_b1000 = bytearray(file_bytes([trace("HHZ", 600, rng=rng)]))
    no_b1000[46:48] = b"\0\0"  # no blockette chain
    bad_time = bytearray(file_bytes([trace("HHZ", 600, rng=rng)]))
    bad_time[22:24] = b"\x03\xe7"  # day 999
    return {"runs past the end": v3[:-5], "CRC": bytes(crc), "no blockette 1000": bytes(no_b1000),
            "implausible start": bytes(bad_time),
            "unsupported identifier": OM.write_mseed3([trace("HHZ", 300, rng=rng)], sid="XFDSN:not_an_fdsn_id")}


@pytest.mark.parametrize("case", list(scanner_error_cases()))
def test_scanner_errors_are_the_scanners(lib, case):
    buf = scanner_error_cases()[case]
    n, kept = C.c_int64(), C.c_int64()
    recs, seg = (_lib.VpMseedRecord * 64)(), (C.c_int64 * 64)()
    rc0 = lib.vp_mseed_scan(buf, len(buf), recs, 64, C.byref(n))
    text0 = _lib.last_error()
    rc1 = lib.vp_mseed_scan_segments(buf, len(buf), recs, seg, 64, C.byref(n), C.byref(kept))
    assert rc0 < 0 and rc1 == rc0 and _lib.last_error() == text0 and kept.value == 0
    with pytest.raises(_lib.VolpickHipError):
        vio.scan_segments(buf)


def test_table_that_does_not_fit_reports_the_count(lib):
    buf = file_bytes([trace("HHZ", 5000, rng=RNG(10))])
    n, kept = C.c_int64(), C.c_int64()
    recs, seg = (_lib.VpMseedRecord * 4)(), (C.c_int64 * 4)()
    assert lib.vp_mseed_scan_segments(buf, len(buf), recs, seg, 4, C.byref(n), C.byref(kept)) == 0
    assert n.value == len(buf) // 512 > 4 and kept.value == 0


# ------------------------------------------------------------------------------------------ plan_file_blocks
def restated_blocks(table, seg, order, rate, in_samples):
    """_group_stream on host traces that hold 1 + their global sample number (0 is then a cell nothing fed)."""
    ns = table["nsamples"].astype(np.int64)
    first, last = vio._segment_ranges(seg)
    base = np.cumsum(ns) - ns
    st = Stream()
    for a, b in zip(first, last):
        n = int(ns[a:b].sum())
        st.append(Trace(np.arange(base[a] + 1, base[a] + 1 + n, dtype=np.float32),
                        dict(network=table["network"][a].decode(), station=table["station"][a].decode(),
                             location=table["location"][a].decode(), channel=table["channel"][a].decode(),
                             starttime=UTCDateTime._from_us(int(table["start_us"][a])), sampling_rate=float(table["sample_rate"][a]))))
    return list(_group_stream(st, order, rate, True, in_samples))


def assert_plan_matches(buf, order="ZNE", rate=100, in_samples=3001):
    """The plan against two expectations.  ``tests/stream_restate.py`` shares no code with the package: it says which blocks
    there are, where they start, what every cell holds and how many runs were too short.  ``_group_stream`` asks the same
    planner as the plan, so agreeing with it says only that ``out_index`` places records where the assembly places samples."""
    table, seg = vio.scan_segments(buf)
    assert int(table["nsamples"].sum()) < 1 << 24  # float32 holds every sample number
    with warnings.catch_warnings(record=True) as w_want:
        warnings.simplefilter("always")
        want = restated_blocks(table, seg, order, rate, in_samples)
    with warnings.catch_warnings(record=True) as w_got:
        warnings.simplefilter("always")
        plan = vio.plan_file_blocks(table, seg, order, rate, in_samples)
    assert plan.reason is None
    assert [str(w.message) for w in w_got] == [str(w.message) for w in w_want] and plan.short_runs == len(w_want)
    got = planned_blocks(table, plan)
    layout = table_layout(table, seg)
    rule = R.restate(layout, order, rate, in_samples)
    assert len(got) == len(rule)
    for b, cells, (trace_id, start_us, data) in zip(plan.blocks, got, rule):
        assert (b["trace_id"], b["start_us"], b["shape"]) == (trace_id, start_us, data.shape)
        assert cells.shape == data.shape and np.array_equal(cells, data)
    assert plan.short_runs == len(w_got) == R.short_runs(layout, order, rate, in_samples)
    assert len(got) == len(want)
    for b, cells, grp in zip(plan.blocks, got, want):
        data = np.asarray(grp["data"])
        assert b["shape"] == data.shape == cells.shape
        assert (b["trace_id"], b["network"], b["station"], b["location"]) == (grp["trace_id"], grp["network"], grp["station"],
                                                                              grp["location"])
        assert b["start_us"] == grp["starttime"]._us
        assert np.array_equal(cells, data)
    return plan


@pytest.mark.parametrize("name", list(layouts()))
@pytest.mark.parametrize("reclen", [256, 4096])
def test_plan_matches_the_assembly(lib, name, reclen):
    assert_plan_matches(layout_bytes(layouts()[name], reclen=reclen))


def test_plan_expected_shapes(lib):
    """The layouts do what their names say (the comparison above would also pass on two empty lists)."""
    L = layouts()
    shapes = lambda name: [b["shape"] for b in assert_plan_matches(layout_bytes(L[name])).blocks]  # noqa: E731
    assert shapes("three_components") == [(3, 7001)]
    assert shapes("gap_splits_two_blocks") == [(3, 7001), (3, 6001)]
    assert shapes("fragment_below_window") == [(3, 7001)]
    assert shapes("two_instruments") == [(3, 7008), (3, 7014), (3, 7001)]  # OTHR.HH, VOLC.EH, VOLC.HH
    plan = assert_plan_matches(layout_bytes(L["fragment_below_window"]))
    assert plan.short_runs == 1 and (plan.out_index < 0).any()


def test_plan_other_component_orders(lib):
    L = layouts()
    for order in ("ZNE", "ENZ", "Z", "NE"):
        assert_plan_matches(layout_bytes(L["names_123"]), order=order)
        assert_plan_matches(layout_bytes(L["late_start_early_end"]), order=order)


def test_plan_mseed3_and_mixed(lib):
    L = layouts()
    assert_plan_matches(layout_bytes(L["gap_in_one_component"], version=3, max_payload=640))
    assert_plan_matches(layout_bytes(L["three_components"][:2]) + layout_bytes(L["three_components"][2:], version=3))


def test_plan_log_channel(lib):
    """A LOG channel is an instrument of its own with no component row: a block of zeros no record feeds, or -- too short for
    the window -- a warning; the data's blocks are untouched either way."""
    data = layout_bytes(layouts()["three_components"])
    plan = assert_plan_matches(data + log_channel_bytes(4000))
    assert [b["offset"] >= 0 for b in plan.blocks] == [True, False]
    plan = assert_plan_matches(log_channel_bytes(1000) + data)
    assert len(plan.blocks) == 1 and plan.short_runs == 1


def test_no_fast_route_is_said(lib):
    rng = RNG(11)
    plan = lambda buf, **kw: vio.plan_file_blocks(*vio.scan_segments(buf), "ZNE", 100, 3001, **kw)  # noqa: E731
    good = layout_bytes(layouts()["three_components"])
    assert plan(good).reason is None
    assert "rate" in plan(file_bytes([trace(c, 4000, rng=rng, rate=50.0) for c in ("HHZ", "HHN", "HHE")])).reason
    assert "rate" in plan(good + file_bytes([trace("BHZ", 4000, rng=rng, rate=20.0)])).reason
    assert "filter" in plan(good, has_filter=True).reason
    assert "overlap" in plan(good + file_bytes([trace("HHZ", 3500, 3000, rng)])).reason
    assert "overlap" in plan(good + file_bytes([trace("HH3", 3500, 3000, rng)])).reason  # another name of the same row
    assert "text" in plan(file_bytes([trace("LOZ", 4000, data=np.full(4000, 65))], encoding=OM.ENC_TEXT)).reason
    assert "no records" in plan(b"").reason
    # ... and what is NOT a reason: an overlap of two components, and of a component the block has no row for
    assert plan(good + file_bytes([trace("HHX", 3500, 3000, rng), trace("HHX", 3500, 5000, rng)])).reason is None


# ------------------------------------------------------------------------------------------ symbols
def test_new_entries_are_declared_exported_and_bound(lib):
    hdr = (ROOT / "include" / "volpick_hip.h").read_text()
    for name in ("vp_mseed_scan_segments", "vp_mseed_decode_on"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl, f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1
    assert f"VP_MSEED_TABLE_BYTES_PER_RECORD = {_lib.VP_MSEED_TABLE_BYTES_PER_RECORD}" in hdr
