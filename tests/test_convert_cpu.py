"""CPU: ``plan_event`` against the numpy restatement of the reference's conversion step (tests/convert_restate.py), ``trim``
on host traces, ``read_many``'s record bookkeeping, the no-trim plan against the existing ``io.stream_to_array``, and the new
symbols in the header, the library and the binding."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import convert_restate as R
from tests.mseed_util import T0, file_bytes, seismogram
from volpick_amd import _lib, generate
from volpick_amd import io as vio
from volpick_amd.convert import plan_event
from volpick_amd.stream import Stream, Trace, UTCDateTime, round_half_away, trim_cut

ROOT = Path(__file__).resolve().parents[1]
BASE = 1_600_000_000_000_000  # microseconds


def make(specs, seed=0):
    """[(channel, offset seconds, npts)] -> (trace dicts for the restatement, Stream of host traces)."""
    rng = np.random.default_rng(seed)
    dicts = [dict(channel=ch, start_us=BASE + int(round(off * 1e6)), rate=100.0,
                  data=rng.integers(-1000, 1000, n).astype(np.int32)) for ch, off, n in specs]
    st = Stream([Trace(d["data"], dict(network="XX", station="S", channel=d["channel"],
                                       starttime=UTCDateTime._from_us(d["start_us"]), sampling_rate=100.0)) for d in dicts])
    return dicts, st


def us(off):
    return None if off is None else BASE + int(round(off * 1e6))


def check(specs, p=None, s=None, **kw):
    """plan_event equals the restatement exactly; returns (plan, restatement)."""
    dicts, st = make(specs)
    before = [(tr.stats.starttime._us, tr.stats.npts) for tr in st]
    plan = plan_event(st, None if p is None else UTCDateTime._from_us(us(p)), None if s is None else UTCDateTime._from_us(us(s)), **kw)
    want = R.restate_event(dicts, us(p), us(s), **kw)
    assert [(tr.stats.starttime._us, tr.stats.npts) for tr in st] == before, "plan_event changed the caller's stream"
    assert plan["samples"] == want["samples"] and plan["starttime"]._us == want["start_us"]
    owner, src = R.plan_owner(plan, list(st))
    assert np.array_equal(owner, want["owner"]) and np.array_equal(src, want["src"])
    assert plan["completeness"] == want["completeness"]
    for name in "ps":
        got, w = plan[f"trace_{name}_arrival_sample"], want[name + "_sample"]
        assert (math.isnan(got) and w is None) or got == w
    for pc in plan["pieces"]:
        assert pc["mean_n"] == pc["source"].stats.npts  # the mean range is the whole untrimmed trace
    return plan, want


def test_float_truncation_of_start_offsets():
    plan, _ = check([("HHZ", 0.0, 200), ("HHN", 0.29, 100), ("HHE", 0.57, 100)], p=0.5, s=1.2)
    assert [pc["dst"] for pc in plan["pieces"]] == [0, 28, 56]  # int(0.29 * 100) = 28, int(0.57 * 100) = 56
    plan, want = check([("HHZ", 0.0, 200), ("HHN", 0.58, 100), ("HHE", 0.57, 100)])
    assert plan["pieces"][1]["dst"] == int(0.58 * 100.0) and plan["pieces"][2]["dst"] == 56


def test_piece_cut_by_the_array_end():
    # the array ends at int(0.29 * 100) + 1 = 29 samples; the N trace starts at sample 1 with 29 samples: 28 fit
    plan, _ = check([("HHZ", 0.0, 5), ("HHN", 0.01, 29), ("HHE", 0.0, 3)])
    n = [pc for pc in plan["pieces"] if pc["component"] == 1][0]
    assert plan["samples"] == 29 and (n["dst"], n["keep_n"], n["mean_n"]) == (1, 28, 29)


@pytest.mark.parametrize("specs", [
    [("HHZ", 0.5, 50), ("HHZ", 0.0, 300), ("HHN", 0.0, 300), ("HHE", 0.0, 300)],                    # shorter first
    [("HHZ", 0.0, 300), ("HHZ", 0.5, 50), ("HHN", 0.0, 300), ("HHE", 0.0, 300)],                    # longer first
    [("HHZ", 0.0, 100), ("HHZ", 0.5, 100), ("HHN", 0.0, 150), ("HHE", 0.0, 150)],                   # equal lengths
    [("HHZ", 0.2, 80), ("HHZ", 0.0, 200), ("HHZ", 1.0, 150), ("HHN", 0.0, 10), ("HHE", 0.0, 10)],   # three, mixed order
    [("HHZ", 1.0, 150), ("HHZ", 0.0, 150), ("HHZ", 0.5, 150), ("HHN", 0.0, 10), ("HHE", 0.0, 10)],  # three equal
])
def test_overlapping_traces_of_one_component(specs):
    plan, _ = check(specs, p=0.7)
    z = [pc["keep_n"] for pc in plan["pieces"] if pc["component"] == 0]
    assert z == sorted(z)  # ascending npts: the longest is written last


def test_missing_component_one_sample_traces_and_channel_codes():
    plan, _ = check([("HHZ", 0.0, 100), ("HHE", 0.1, 100)], s=0.3)
    assert {pc["component"] for pc in plan["pieces"]} == {0, 2} and plan["completeness"] < 2 / 3 + 1e-12
    check([("HHZ", 0.0, 1), ("HHN", 0.0, 1), ("HHE", 0.0, 1)], p=0.0)
    check([("HHZ", 0.0, 1), ("HHN", 0.05, 1)])
    plan, _ = check([("Z", 0.0, 40), ("HHZ", 0.1, 50), ("EHZ1", 0.0, 500), ("N", 0.0, 30), ("EHE", 0.0, 30)])
    assert len([pc for pc in plan["pieces"] if pc["component"] == 0]) == 2  # "EHZ1" matches no component
    assert plan["samples"] == 500  # ... but its span still sets the array's extent, as in the reference


@pytest.mark.parametrize("npts,cut", [(9000, False), (9001, False), (9002, True)])
def test_cut_bounds_branch(npts, cut):
    # 3 * 10 + 60 = 90 s: 89.99 s and exactly 90 s are kept whole, 90.01 s is trimmed by 10 s at both ends
    plan, _ = check([("HHZ", 0.0, npts), ("HHN", 0.0, npts), ("HHE", 0.004, npts - 7)], p=30.0, s=40.0, cut_bounds=10)
    assert (plan["samples"] < npts - 1500) == cut
    z = plan["pieces"][0]
    assert (z["keep_lo"], z["keep_n"]) == ((1000, npts - 2000) if cut else (0, npts)) and z["mean_n"] == npts


def test_cut_bounds_trims_a_trace_away_entirely():
    plan, _ = check([("HHZ", 0.0, 9500), ("HHZ", 0.0, 300), ("HHN", 0.0, 9500), ("HHE", 94.0, 100)], cut_bounds=10)
    assert len(plan["pieces"]) == 2  # the short Z trace and the late E trace are gone


@pytest.mark.parametrize("p,s", [(60.0, None), (None, 120.0), (60.0, 120.0)])
def test_check_long_traces_branch(p, s):
    specs = [("HHZ", 0.0, 25001), ("HHN", 0.0, 25001), ("HHE", 0.3, 24000)]
    plan, _ = check(specs, p=p, s=s, check_long_traces=True)
    assert plan["samples"] < 25001
    whole, _ = check(specs, p=p, s=s, check_long_traces=True, check_long_traces_limit=300)  # 250 s: not taken
    assert whole["samples"] == 25001
    both, _ = check(specs, p=p, s=s, cut_bounds=20, check_long_traces=True)
    assert both["samples"] <= plan["samples"]


def test_missing_times():
    plan, _ = check([("HHZ", 0.0, 100), ("HHN", 0.0, 100), ("HHE", 0.0, 100)])
    assert math.isnan(plan["trace_p_arrival_sample"]) and math.isnan(plan["trace_s_arrival_sample"])
    _, st = make([("HHZ", 0.0, 100)])
    for nothing in (None, float("nan"), np.datetime64("NaT")):
        assert math.isnan(plan_event(st, nothing, "2020-09-13T12:26:40.5")["trace_p_arrival_sample"])
    assert plan_event(st, nothing, "2020-09-13T12:26:40.5")["trace_s_arrival_sample"] == 50.0
    with pytest.raises(ValueError, match="P or an S"):
        plan_event(make([("HHZ", 0.0, 20001)])[1], None, None, check_long_traces=True)
    masked = Stream([Trace(np.ma.masked_array(np.arange(5.0), mask=[0, 1, 0, 0, 0]), dict(channel="HHZ", sampling_rate=100.0))])
    with pytest.raises(NotImplementedError, match="masked traces cannot be"):
        plan_event(masked, None, None)


# ------------------------------------------------------------------------------------------------------------- trim
TRIM_TIMES = [0.10, 0.105, 0.095, 0.1049, 0.1051, -1.0, 0.0, 0.99, 0.995, 5.0]


def test_round_half_away():
    assert [round_half_away(v) for v in (2.5, -2.5, 0.5, -0.5, 0.49, 10.5, -10.4)] == [3, -3, 1, -1, 0, 11, -10]


@pytest.mark.parametrize("t0", [None] + TRIM_TIMES)
@pytest.mark.parametrize("t1", [None] + TRIM_TIMES)
def test_trim_host_traces_against_the_restatement(t0, t1):
    (d,), st = make([("HHZ", 0.0, 100)])
    want = R.trim_one(dict(start_us=d["start_us"], rate=100.0, first=0, n=100), us(t0), us(t1))
    tr = st[0]
    a0 = None if t0 is None else UTCDateTime._from_us(us(t0))
    a1 = None if t1 is None else UTCDateTime._from_us(us(t1))
    assert tr.trim(a0, a1) is tr
    assert tr.stats.npts == want["n"] == len(tr.data)
    assert np.array_equal(tr.data, d["data"][want["first"]:want["first"] + want["n"]])
    if want["n"]:
        assert tr.stats.starttime._us == want["start_us"]
    assert trim_cut(UTCDateTime._from_us(d["start_us"]), 100, 100.0, a0, a1) == (want["first"] if want["n"] or want["first"] else 0, want["n"])


def test_trim_known_answers_and_stream_trim():
    def cut(t0, t1):
        return trim_cut(UTCDateTime._from_us(BASE), 100, 100.0, None if t0 is None else UTCDateTime._from_us(us(t0)),
                        None if t1 is None else UTCDateTime._from_us(us(t1)))

    assert cut(0.10, None) == (10, 90) and cut(0.104, None) == (10, 90) and cut(0.106, None) == (11, 89)
    assert cut(-3.0, None) == (0, 100) and cut(None, 7.0) == (0, 100)           # before the start, after the end: no cut
    assert cut(None, 0.50) == (0, 51) and cut(None, 0.504) == (0, 51) and cut(None, 0.506) == (0, 52)
    assert cut(0.10, 0.50) == (10, 41)
    assert cut(0.60, 0.50)[1] == 0 and cut(2.0, None)[1] == 0 and cut(None, -1.0)[1] == 0   # nothing left
    _, st = make([("HHZ", 0.0, 100), ("HHN", 0.5, 100), ("HHE", 2.0, 10)])
    assert st.trim(UTCDateTime._from_us(us(0.2)), UTCDateTime._from_us(us(1.2))) is st
    assert [(tr.stats.channel, tr.stats.npts, tr.stats.starttime._us) for tr in st] == [("HHZ", 80, us(0.2)), ("HHN", 71, us(0.5))]


# -------------------------------------------------------------------------------------------------------- read_many
def test_read_many_bookkeeping(lib):
    rng = np.random.default_rng(3)
    x = seismogram(3000, rng)
    tr = dict(network="XX", station="ONE", location="", channel="HHZ", start_us=T0, rate=100.0)
    a = file_bytes([dict(tr, data=x[:1500])])
    b = file_bytes([dict(tr, data=x[1500:], start_us=T0 + 15_000_000)])  # continues file a's trace without a gap
    c = file_bytes([dict(tr, data=x[:700].astype(np.float32), channel="HHN")], encoding=4)
    bufs = [a, b, c]
    table, seg, bounds, bases = vio.many_tables(bufs)
    assert list(bases) == [0, len(a), len(a) + len(b)] and bounds[-1] == len(table)
    for k, buf in enumerate(bufs):
        r, s = vio._segments(vio.scan_mseed(buf))
        mine = table[bounds[k]:bounds[k + 1]]
        assert np.array_equal(mine["offset"] - bases[k], r["offset"])
        for f in ("start_us", "nsamples", "encoding", "channel"):
            assert np.array_equal(mine[f], r[f])
        assert np.array_equal(seg[bounds[k]:bounds[k + 1]] - seg[bounds[k]], s)  # chained as the file alone is
        joined = b"".join(bufs)
        for rec in mine[:2]:
            assert joined[rec["offset"]:rec["offset"] + 6] == buf[rec["offset"] - bases[k]:rec["offset"] - bases[k] + 6]
    # a and b would chain into one segment in one file; across two files they do not
    _, s_ab = vio._segments(vio.scan_mseed(a + b))
    assert len(np.unique(s_ab)) == 1
    assert seg[bounds[1]] != seg[bounds[1] - 1] and len(np.unique(seg)) == 3
    # a short payload is named with the offset within its own file
    status = np.zeros(len(table), np.int32)
    assert vio.short_payload_error(table, status, bounds, bases) is None
    status[bounds[1] + 2] = 2
    err = vio.short_payload_error(table, status, bounds, bases)
    assert isinstance(err, ValueError) and f"at byte {2 * 512}:" in str(err) and "fewer samples" in str(err)


# ----------------------------------------------------------------------------------------- the no-trim plan in numpy
@pytest.mark.parametrize("specs", [
    [("HHZ", 0.0, 200), ("HHN", 0.29, 100), ("HHE", 0.57, 100)],
    [("HHZ", 0.5, 50), ("HHZ", 0.0, 300), ("HHZ", 1.0, 300), ("HHE", 0.0, 30)],
    [("HHZ", 0.0, 5), ("HHN", 0.01, 29), ("HHE", 0.0, 3)],
])
def test_no_trim_plan_reproduces_stream_to_array(specs):
    _, st = make(specs, seed=5)
    plan = plan_event(st, None, None)
    data = np.zeros((3, plan["samples"]))
    for pc in plan["pieces"]:
        x = pc["source"].data.astype(np.float64)
        data[pc["component"], pc["dst"]:pc["dst"] + pc["keep_n"]] = (x - x.mean())[pc["keep_lo"]:pc["keep_lo"] + pc["keep_n"]]
    data -= np.mean(data, axis=1, keepdims=True)
    start, want, completeness = vio.stream_to_array(st.copy().detrend("demean"))
    assert start == plan["starttime"] and completeness == plan["completeness"]
    assert np.array_equal(data, want)


# ---------------------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "volpick_hip.h").read_text()
    for name in ("vp_bank_assemble", "vp_bank_read"):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported"
    source = (ROOT / "volpick_amd" / "csrc" / "assemble.hip").read_text()
    assert re.search(r"#define VP_ASSEMBLE_TILE 4096\b", header) and _lib.VP_ASSEMBLE_TILE == 4096
    assert "AS_TILE == VP_ASSEMBLE_TILE" in source and re.search(r"AS_NTH = 256, AS_PER = 16", source)
    assert generate.ASSEMBLE_PIECE.itemsize == C.sizeof(_lib.VpAssemblePiece) == 56
    assert "assemble.hip" in (ROOT / "volpick_amd" / "csrc" / "Makefile").read_text()


def test_null_arguments_are_refused_without_a_device(lib):
    assert lib.vp_bank_assemble(None, 0, 1, None, 0, None, None, None) == -1 and b"vp_bank_assemble" in lib.vp_last_error()
    out = np.full(3, -7.0, np.float32)
    assert lib.vp_bank_read(None, 0, out.ctypes.data_as(C.c_void_p), 0) == -1 and b"null" in lib.vp_last_error()
    assert (out == -7.0).all()
