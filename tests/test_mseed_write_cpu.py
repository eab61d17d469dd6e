"""The host side of the miniSEED writer, without a GPU: the 64-byte record headers (``vp_mseed_record_headers`` and the
stand-alone build of ``mseed_write_host.h``) against the oracle's ``write_mseed``, the SEED rate fields against
``oracle.mseed.sample_rate``, and every argument rule of ``volpick_amd.io.write_mseed`` (``plan_write``).

Rate fields: the oracle's writer stores ``(rate, 1)`` for an integer rate and ``(-round(1 / rate), 1)`` otherwise, which
is not the rate for 62.5 Hz (it stores a factor of 0) and is another exact pair for 0.1 Hz (``(-10, 1)``; the writer's rule
finds ``(1, -10)`` first).  Where the two pairs differ the four rate bytes are compared with the writer's own rule and the
other sixty with the oracle."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
from datetime import datetime, timezone
from pathlib import Path

import numpy as np
import pytest

from oracle import mseed as OM
from volpick_amd import _lib
from volpick_amd import io as VIO
from volpick_amd.stream import Stream, Trace, UTCDateTime

ROOT = Path(__file__).resolve().parents[1]


def us_of(*ymdhms, us=0):
    d = datetime(*ymdhms, tzinfo=timezone.utc) - datetime(1970, 1, 1, tzinfo=timezone.utc)
    return (d.days * 86400 + d.seconds) * 1_000_000 + us


# (name, start_us, rate): record starts that cross midnight, cross the year, fall on 29 February and on day 366
STARTS = [
    ("plain", 1_600_000_000_123_400, 100.0),
    ("midnight", us_of(2021, 6, 30, 23, 59, 59, us=900_000), 100.0),
    ("new_year", us_of(2021, 12, 31, 23, 59, 59, us=700_000), 100.0),
    ("feb_29", us_of(2020, 2, 28, 23, 59, 59, us=950_000), 100.0),
    ("day_366", us_of(2020, 12, 30, 23, 59, 59, us=990_000), 40.0),
    ("off_grid", 1_600_000_000_123_456, 100.0),
    ("before_1970", us_of(1969, 12, 31, 23, 59, 59, us=500_000), 100.0),
]
RATES = [100.0, 40.0, 1.0, 0.1, 62.5, 200.0]
PAIRS = {100.0: (100, 1), 40.0: (40, 1), 1.0: (1, 1), 0.1: (1, -10), 62.5: (125, -2), 200.0: (200, 1)}


def oracle_pair(rate):
    """The pair ``oracle.mseed.write_mseed`` stores."""
    return (int(rate), 1) if rate >= 1 and rate == int(rate) else (-int(round(1.0 / rate)), 1)


def c_trace(tr):
    t = _lib.VpMseedTrace()
    t.start_us, t.sample_rate, t.first_sample, t.nsamples, t.quality = tr["start_us"], tr["rate"], 0, len(tr["data"]), ord("D")
    for f in ("network", "station", "location", "channel"):
        setattr(t, f, tr[f].encode())
    return t


def headers(lib, tr, first, count, seq0, reclen, enc, be, mode):
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    out = np.full(64 * len(first) + 8, 0xAB, np.uint8)
    t = c_trace(tr)
    rc = lib.vp_mseed_record_headers(C.byref(t), first.ctypes.data_as(C.POINTER(C.c_int64)), count.ctypes.data_as(C.POINTER(C.c_int64)),
                                     len(first), seq0, reclen, enc, int(be), mode, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.vp_last_error()
    assert (out[64 * len(first):] == 0xAB).all()
    return out[:64 * len(first)].reshape(-1, 64)


def check_against_oracle(got, buf, reclen, rate, be):
    """``got``: (n, 64) header bytes; ``buf``: the oracle's file."""
    want = np.frombuffer(buf, np.uint8).reshape(-1, reclen)[:, :64]
    assert got.shape == want.shape
    same_pair = oracle_pair(rate) == PAIRS.get(rate, oracle_pair(rate))
    keep = np.ones(64, bool)
    if not same_pair:
        keep[32:36] = False
        for h in got:
            assert struct.unpack_from((">" if be else "<") + "hh", h.tobytes(), 32) == PAIRS[rate]
    bad = np.argwhere(got[:, keep] != want[:, keep])
    assert len(bad) == 0, f"first differing (record, byte among the compared): {bad[0]}"


def trace_dict(start_us, rate, n, cha="HHZ", sta="VOLC"):
    return dict(network="XX", station=sta, location="00", channel=cha, start_us=start_us, rate=rate,
                data=np.arange(n, dtype=np.int32))


@pytest.mark.parametrize("be", [True, False])
@pytest.mark.parametrize("b1001", [False, True])
def test_headers_equal_the_oracles(lib, be, b1001):
    reclen, per = 128, 16  # int32 records of 16 samples: the record table is known without a packer
    for name, start_us, rate in STARTS:
        tr = trace_dict(start_us, rate, 16 * 9 + 5)
        buf = OM.write_mseed([tr], reclen=reclen, encoding=3, byteorder=">" if be else "<", with_b1001=b1001)
        first = np.arange(0, len(tr["data"]), per)
        count = np.minimum(per, len(tr["data"]) - first)
        got = headers(lib, tr, first, count, 1, reclen, 3, be, int(b1001))
        check_against_oracle(got, buf, reclen, rate, be)
    # the record starts do what their names say
    t = [OM.us_to_btime(us_of(2020, 2, 28, 23, 59, 59, us=950_000) + k * 160_000) for k in range(10)]
    assert (t[0][0], t[0][1]) == (2020, 59) and (t[-1][0], t[-1][1]) == (2020, 60)
    t = [OM.us_to_btime(us_of(2020, 12, 30, 23, 59, 59, us=990_000) + k * 400_000) for k in range(10)]
    assert t[0][1] == 365 and t[-1][1] == 366


@pytest.mark.parametrize("rate", RATES)
def test_headers_at_every_rate(lib, rate):
    for be in (True, False):
        tr = trace_dict(1_600_000_000_123_400, rate, 40)
        buf = OM.write_mseed([tr], reclen=128, encoding=3, byteorder=">" if be else "<")
        got = headers(lib, tr, [0, 16, 32], [16, 16, 8], 1, 128, 3, be, 0)
        check_against_oracle(got, buf, 128, rate, be)
    assert VIO.rate_fields(rate) == PAIRS[rate]
    assert OM.sample_rate(*PAIRS[rate]) == rate


def test_blockette_1001_when_a_start_is_off_the_grid(lib):
    on, off = trace_dict(1_600_000_000_123_400, 100.0, 40), trace_dict(1_600_000_000_123_456, 100.0, 40)
    first, count = [0, 16, 32], [16, 16, 8]
    for tr, wants in ((on, False), (off, True)):
        buf = OM.write_mseed([tr], reclen=128, encoding=3, with_b1001=wants)
        check_against_oracle(headers(lib, tr, first, count, 1, 128, 3, True, -1), buf, 128, 100.0, True)
    # 3 Hz: only the second record starts off the 100 us grid (16 / 3 s), and then every record of the trace carries it
    third = trace_dict(1_600_000_000_000_000, 3.0, 40)
    got = headers(lib, third, first, count, 1, 128, 3, True, -1)
    buf = OM.write_mseed([third], reclen=128, encoding=3, with_b1001=True)
    check_against_oracle(got, buf, 128, 3.0, True)
    assert got[0, 39] == 2 and got[0, 61] == 0 and got[1, 61] == 33
    # frame counts, and forced on for Steim records
    st = headers(lib, on, [0], [40], 1, 512, 11, True, 1)
    assert st[0, 63] == 7 and st[0, 52] == 11 and st[0, 54] == 9


def test_sequence_numbers_run_across_traces(lib):
    a, b = trace_dict(1_600_000_000_123_400, 100.0, 40, "HHZ"), trace_dict(1_600_000_100_000_000, 100.0, 20, "HHN", "VOLCA")
    buf = OM.write_mseed([a, b], reclen=128, encoding=3)
    got = np.concatenate([headers(lib, a, [0, 16, 32], [16, 16, 8], 1, 128, 3, True, 0),
                          headers(lib, b, [0, 16], [16, 4], 4, 128, 3, True, 0)])
    check_against_oracle(got, buf, 128, 100.0, True)
    assert [bytes(h[:6]) for h in got] == [b"000001", b"000002", b"000003", b"000004", b"000005"]
    wrap = headers(lib, a, [0, 16], [16, 16], 999_999, 128, 3, True, 0)
    assert [bytes(h[:6]) for h in wrap] == [b"999999", b"000000"]
    assert bytes(wrap[0]) == OM.write_mseed([a], reclen=128, encoding=3, seq0=999_999)[:64]


def test_header_refusals(lib):
    tr = trace_dict(0, 100.0, 4)
    one = np.array([0], np.int64)
    p = one.ctypes.data_as(C.POINTER(C.c_int64))
    out = np.zeros(64, np.uint8)
    o = out.ctypes.data_as(C.c_void_p)
    t = c_trace(tr)
    assert lib.vp_mseed_record_headers(C.byref(t), p, p, 1, 1, 100, 3, 1, 0, o) == -1 and b"reclen" in lib.vp_last_error()
    assert lib.vp_mseed_record_headers(C.byref(t), p, p, 1, 1, 128, 2, 1, 0, o) == -1 and b"encoding" in lib.vp_last_error()
    assert lib.vp_mseed_record_headers(C.byref(t), p, p, 1, 1, 65536, 11, 1, 0, o) == -4
    big = np.array([65536], np.int64)
    assert lib.vp_mseed_record_headers(C.byref(t), p, big.ctypes.data_as(C.POINTER(C.c_int64)), 1, 1, 128, 3, 1, 0, o) == -1
    t.sample_rate = 1e-5
    assert lib.vp_mseed_record_headers(C.byref(t), p, p, 1, 1, 128, 3, 1, 0, o) == -1 and b"rate" in lib.vp_last_error()
    assert (out == 0).all()
    # the encoder refuses the same arguments before it touches a device
    n = C.c_size_t(7)
    r, bt, bs = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    t = c_trace(tr)
    args = (C.byref(n), C.byref(r), C.byref(bt), C.byref(bs))
    assert lib.vp_mseed_encode(0, o, 0, 0, C.byref(t), 1, 100, 11, 1, -1, o, 64, *args) == -1 and b"reclen" in lib.vp_last_error()
    assert lib.vp_mseed_encode(0, o, 0, 1, C.byref(t), 1, 512, 11, 1, -1, o, 64, *args) == -1 and b"encoding" in lib.vp_last_error()
    assert lib.vp_mseed_encode(0, o, 0, 0, C.byref(t), 1, 65536, 11, 1, -1, o, 64, *args) == -4
    t.station = b"VOLCAN"
    assert lib.vp_mseed_encode(0, o, 0, 0, C.byref(t), 1, 512, 11, 1, -1, o, 64, *args) == -1 and b"station" in lib.vp_last_error()
    assert (n.value, r.value, bt.value, bs.value) == (0, 0, -1, -1) and (out == 0).all()


def test_rate_rule_on_a_grid(lib):
    """Every pair gives the rate back exactly under the oracle's rule, or the rate is refused."""
    rates = [k / m for k in (1, 2, 3, 5, 7, 20, 25, 40, 50, 100, 125, 250, 1000, 4000, 32767) for m in (1, 2, 3, 4, 5, 7, 8, 10, 16, 100, 3600)]
    rates += [1 / k for k in (1, 2, 10, 60, 3600, 32767, 32768)] + [32768.0, 1e-5, 19.99, np.pi, 0.3, 99.99999999999999]
    given = refused = 0
    for rate in rates:
        try:
            f, m = VIO.rate_fields(rate)
        except ValueError:
            refused += 1
            continue
        given += 1
        assert -32768 <= f <= 32767 and f != 0 and -32767 <= m <= 32767 and m != 0
        assert OM.sample_rate(f, m) == rate, (rate, f, m)
        if f > 0:  # the smallest multiplier
            assert all(rate * k != np.floor(rate * k) or rate * k > 32767 or rate * k < 1 or (rate * k) / k != rate for k in range(1, -m if m < 0 else 1))
    assert given > 100 and refused >= 4
    for rate in (0.0, -1.0, float("nan"), float("inf"), 32768.0, 1e-5, np.pi):
        with pytest.raises(ValueError, match="factor / multiplier"):
            VIO.rate_fields(rate)
    assert VIO.rate_fields(1 / 3600) == (1, -3600) and VIO.rate_fields(1 / 3) == (1, -3)
    assert (1 / 49) * 49 != 1.0 and VIO.rate_fields(1 / 49) == (5, -245)  # the first product that is an integer and exact


def host_trace(data, rate=100.0, mseed=None, **hdr):
    h = dict(network="XX", station="VOLC", location="", channel="HHZ", starttime=UTCDateTime(1_600_000_000.0), sampling_rate=rate)
    h.update(hdr)
    tr = Trace(np.asanyarray(data), h)
    if mseed is not None:
        tr.stats["mseed"] = dict(mseed)
    return tr


def test_defaults_and_the_encoding_table(lib):
    i32, i16 = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int16)
    f32, f64 = np.arange(5, dtype=np.float32), np.arange(5, dtype=np.float64)
    for data, dtype, enc, kind in ((i32, "int32", 11, 0), (i16, "int16", 1, 0), (f32, "float32", 4, 1), (f64, "float64", 5, 2)):
        (p,) = VIO.plan_write(host_trace(data))
        assert (p["dtype"], p["encoding"], p["kind"], p["reclen"], p["byteorder"], p["dataquality"]) == (dtype, enc, kind, 4096, ">", "D")
        assert (p["factor"], p["multiplier"]) == (100, 1)
    # stats.mseed, as read() records it, wins over the defaults; a keyword wins over both
    was = dict(encoding=10, byteorder="<", record_length=512, dataquality="Q", number_of_records=3)
    (p,) = VIO.plan_write(Stream([host_trace(i32, mseed=was)]))
    assert (p["encoding"], p["reclen"], p["byteorder"], p["dataquality"]) == (10, 512, "<", "Q")
    (p,) = VIO.plan_write(host_trace(i32, mseed=was), reclen=256, encoding=3, byteorder=">", dataquality="M")
    assert (p["encoding"], p["reclen"], p["byteorder"], p["dataquality"]) == (3, 256, ">", "M")
    assert VIO.plan_write(host_trace(i32), byteorder=0)[0]["byteorder"] == "<" and VIO.plan_write(host_trace(i32), byteorder=1)[0]["byteorder"] == ">"
    # an encoding of stats.mseed that no longer matches the sample type gives way to the type's default
    (p,) = VIO.plan_write(host_trace(f32, mseed=dict(encoding=11, byteorder=">", record_length=512, dataquality="D")))
    assert (p["encoding"], p["reclen"]) == (4, 512)
    (p,) = VIO.plan_write(host_trace(i32, mseed=dict(encoding=4, byteorder="<", record_length=1000, dataquality="")))
    assert (p["encoding"], p["reclen"], p["byteorder"], p["dataquality"]) == (11, 4096, "<", "D")  # (a miniSEED 3 trace)
    # the table
    for data, allowed in ((i32, (11, 10, 3, 1)), (i16, (1,)), (f32, (4,)), (f64, (5,))):
        for enc in (0, 1, 2, 3, 4, 5, 10, 11, 12):
            if enc in allowed:
                assert VIO.plan_write(host_trace(data), encoding=enc)[0]["encoding"] == enc
            else:
                with pytest.raises(ValueError, match=f"encoding {enc} cannot hold"):
                    VIO.plan_write(host_trace(data), encoding=enc)
    # empty traces are skipped, order is kept, a Trace and a Stream are both taken
    st = Stream([host_trace(i32, channel="HHZ"), host_trace(np.zeros(0, np.int32), channel="HHN"), host_trace(f32, channel="HHE")])
    assert [p["trace"].stats.channel for p in VIO.plan_write(st)] == ["HHZ", "HHE"]
    assert VIO.plan_write(Stream()) == []


def test_refusals_by_message(lib, tmp_path):
    i32 = np.arange(5, dtype=np.int32)
    cases = [
        (host_trace(np.arange(5, dtype=np.int64)), {}, "type int64 cannot be written"),
        (host_trace(np.arange(5, dtype=np.uint8)), {}, "type uint8 cannot be written"),
        (host_trace(np.array([b"a", b"b"], "S1")), {}, "text records are not written"),
        (host_trace(np.ma.masked_array(i32, mask=[0, 1, 0, 0, 0])), {}, "masked traces cannot be written"),
        (host_trace(i32), dict(encoding=2), "encoding 2 cannot hold int32"),
        (host_trace(i32), dict(encoding=0), "encoding 0 cannot hold"),
        (host_trace(i32), dict(reclen=64), "reclen 64 is not a power of two in 128..65536"),
        (host_trace(i32), dict(reclen=1000), "reclen 1000 is not a power of two"),
        (host_trace(i32), dict(reclen=131072), "reclen 131072 is not a power of two in 128..65536"),
        (host_trace(i32), dict(reclen=65536), "reclen 65536 with encoding 11"),
        (host_trace(i32), dict(byteorder="="), "byteorder '=' is none of"),
        (host_trace(i32), dict(dataquality="X"), "dataquality 'X' is none of D, R, Q, M"),
        (host_trace(i32, network="XXX"), {}, "network 'XXX' is longer than 2 characters"),
        (host_trace(i32, station="VOLCAN"), {}, "station 'VOLCAN' is longer than 5 characters"),
        (host_trace(i32, location="000"), {}, "location '000' is longer than 2 characters"),
        (host_trace(i32, channel="HHZZ"), {}, "channel 'HHZZ' is longer than 3 characters"),
        (host_trace(i32, rate=0.0), {}, "sampling rate 0.0 is not positive"),
        (host_trace(i32, rate=-5.0), {}, "sampling rate -5.0 is not positive"),
        (host_trace(i32, rate=1e-5), {}, "no exact SEED factor / multiplier pair"),
    ]
    target = tmp_path / "never.mseed"
    for tr, kw, message in cases:
        with pytest.raises(ValueError, match=re.escape(message)):
            VIO.write_mseed(Stream([host_trace(i32), tr]), target, **kw)  # refused although a good trace comes first
        with pytest.raises(ValueError, match=re.escape(message)):
            tr.write(target, **kw)
    assert not target.exists()
    for fmt in ("SAC", "mseed3", "GSE2"):
        with pytest.raises(ValueError, match="unsupported output format"):
            Stream([host_trace(i32)]).write(target, format=fmt)
        with pytest.raises(ValueError, match="unsupported output format"):
            host_trace(i32).write(target, format=fmt)
    assert VIO.plan_write(host_trace(i32), reclen=65536, encoding=10)[0]["reclen"] == 65536


def test_symbols_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "volpick_hip.h").read_text()
    for name in ("vp_mseed_encode", "vp_mseed_rate_fields", "vp_mseed_record_headers", "vp_mseed_encode_bench",
                 "vp_mseed_encode_release_scratch"):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(rf"enum \{{ VP_MSEED_ENCODE_CHUNK = {_lib.VP_MSEED_ENCODE_CHUNK} \}};", header)
    assert re.search(rf"enum \{{ VP_MSEED_ENCODE_STAGES = {_lib.VP_MSEED_ENCODE_STAGES} \}};", header)
    assert C.sizeof(_lib.VpMseedTrace) == 56
    import volpick_amd

    assert volpick_amd.write_mseed is VIO.write_mseed


def test_host_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/llvm/bin/clang++")
    exe = tmp_path / "mseed_write_host_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-I", str(ROOT / "volpick_amd" / "csrc"),
           str(ROOT / "tests" / "mseed_write_host_check.cpp"), "-o", str(exe)]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + sanitize, capture_output=True).returncode != 0:  # no sanitizer runtime for this compiler
        print("sanitizer build failed; building without")
        subprocess.run(cmd, check=True)
    # one record each: (start, rate, first sample, count, sequence, reclen, encoding, big-endian, b1001 mode)
    jobs, want = [], []
    for name, start_us, rate in STARTS:
        for first in (0, 16, 9 * 16):
            for be in (1, 0):
                mode = -1 if name == "off_grid" else first % 2
                b1001 = start_us % 100 != 0 if mode == -1 else bool(mode)
                tr = trace_dict(start_us, rate, first + 16)
                buf = OM.write_mseed([tr], reclen=128, encoding=3, byteorder=">" if be else "<", with_b1001=b1001)
                want.append(buf[128 * (first // 16): 128 * (first // 16) + 64])
                jobs.append((start_us, repr(rate), first, 16, first // 16 + 1, 128, 3, be, mode))
    jobs.append((0, "62.5", 0, 7, 1, 512, 11, 1, 1))
    jobs.append((0, "1e-5", 0, 7, 1, 512, 11, 1, 1))
    r = subprocess.run([str(exe)] + [str(v) for j in jobs for v in j], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for k, w in enumerate(want):
        assert lines[k] == "header " + w.hex(), (jobs[k], lines[k])
    h = bytes.fromhex(lines[len(want)].split()[1])
    assert struct.unpack_from(">hh", h, 32) == (125, -2) and h[52] == 11 and h[63] == 7 and h[39] == 2
    assert lines[len(want) + 1] == "refused -1"
    codes = dict(ln.split()[1:] for ln in lines[len(jobs):])
    assert len(codes) == 23
    for name, code in codes.items():
        assert int(code) == (0 if name.startswith("valid") else -4 if name == "steim2_65536" else -1), name
