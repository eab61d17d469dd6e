"""``volpick_amd.io.write_mseed`` on the GPU against the oracle's encoder: whole files, byte for byte, no tolerances.

``L`` is the packer's chunk (``VP_MSEED_ENCODE_CHUNK``); lengths and positions straddle it, its sub-chunks of 256 samples and
the records' word counts (13 at 128 bytes, 103 at 512, 943 at 4096).  The oracle costs about 7.5 us per sample, so the
byte-exact cases stay below 300,000 samples in total; the round trip through ``read`` needs no oracle."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from oracle import mseed as OM
from tests.mseed_util import T0, seismogram
from volpick_amd import _lib, read, write_mseed
from volpick_amd import io as VIO
from volpick_amd.stream import Stream, Trace, UTCDateTime

pytestmark = pytest.mark.gpu
L = _lib.VP_MSEED_ENCODE_CHUNK
LENGTHS = [1, 2, 6, 7, 8, 91, 92, 103 * 7 - 1, 103 * 7 + 1, L - 1, L, L + 1, 2 * L + 3, 3 * L + 5]
EDGES = [-8, 7, 8, -9, -16, 15, 16, -17, 31, -32, 32, 127, -128, 128, 511, -512, 512, 16383, -16384, 16384,
         (1 << 29) - 1, -(1 << 29) + 1, -(1 << 29)]


@pytest.fixture(scope="module", autouse=True)
def scratch_released_afterwards():
    """The writer's scratch is per device and grow-only: what this module made it grow to is not left to the rest of the suite."""
    yield
    VIO.release_encode_scratch()


def trace_dict(data, k=0, start_us=T0, rate=100.0, sta="VOLC"):
    return dict(network="XX", station=sta, location="", channel=f"H{k // 10 % 10}{k % 10}", start_us=start_us, rate=rate,
                data=np.asarray(data))


def stream_of(dicts, device=True):
    st = Stream()
    for d in dicts:
        hdr = dict(network=d["network"], station=d["station"], location=d["location"], channel=d["channel"],
                   starttime=UTCDateTime._from_us(d["start_us"]), sampling_rate=d["rate"])
        if device:
            st.append(Trace(header=hdr, device_data=torch.from_numpy(np.ascontiguousarray(d["data"])).cuda()))
        else:
            st.append(Trace(d["data"], hdr))
    return st


def assert_same_file(got, want, reclen):
    assert len(got) == len(want), (len(got), len(want))
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"first differing byte: record {at // reclen}, byte {at % reclen} (word {(at % reclen - 64) // 4} of the "
                             f"data): {a[at]} != {b[at]}; {int((a != b).sum())} bytes differ")


def check(dicts, reclen, encoding, byteorder, with_b1001=False):
    st = stream_of(dicts)
    got = write_mseed(st, reclen=reclen, encoding=encoding, byteorder=byteorder, blockette1001=with_b1001)
    assert all(tr._data is None for tr in st)  # read where they lie: no host copy
    assert_same_file(got, OM.write_mseed(dicts, reclen=reclen, encoding=encoding, byteorder=byteorder, with_b1001=with_b1001), reclen)


def walk(n, rng, version):
    """Kind (a): a seismogram, for Steim-2 without spikes and with the first sample inside 30 bits."""
    x = seismogram(n, rng, spikes=version == 1)
    x[0] %= 1000
    return x


@pytest.mark.parametrize("encoding,byteorder,reclen", [(e, b, r) for e in (11, 10) for b, r in ((">", 128), (">", 512), (">", 4096), ("<", 512))])
def test_seismograms_of_every_length(encoding, byteorder, reclen):
    rng = np.random.default_rng(100 * encoding + reclen)
    dicts = [trace_dict(walk(n, rng, encoding - 9), k) for k, n in enumerate(LENGTHS)]
    check(dicts, reclen, encoding, byteorder)  # one call, one set of launches
    for k in (0, 3, 9):  # and alone
        check([dicts[k]], reclen, encoding, byteorder)


@pytest.mark.parametrize("encoding", [11, 10])
def test_constant_traces_keep_every_entry_chain_apart(encoding):
    """Every word takes 7 (Steim-1: 4) differences, so the chains that enter a chunk at different offsets never merge: a
    wrong entry offset shifts every word behind it."""
    step = 7 if encoding == 11 else 4
    lengths = [L + r for r in range(-2, step - 2)] + [2 * L - 1, 2 * L, 2 * L + 3]
    dicts = [trace_dict(np.full(n, 5, np.int32), k) for k, n in enumerate(lengths)]
    assert sorted({n % step for n in lengths}) == list(range(step))
    check(dicts, 128, encoding, ">")
    check(dicts[:3], 512, encoding, "<")


@pytest.mark.parametrize("encoding", [11, 10])
def test_class_edges_wraps_and_tails(encoding):
    rng = np.random.default_rng(encoding)
    edges = np.array(EDGES if encoding == 11 else EDGES + [32767, -32768, 32768, -32769, (1 << 31) - 1, -(1 << 31)], np.int64)
    d = rng.choice(edges, 2 * L + 3)
    d[0] = 17
    x = np.cumsum(d).astype(np.uint64).astype(np.uint32).view(np.int32)  # the sums wrap, the differences are the edges
    check([trace_dict(x)], 512, encoding, ">")
    check([trace_dict(x)], 128, encoding, "<")
    # up to 2^31 - 1 in steps inside 30 bits, then on to -2^31: the difference wraps to 1
    top = np.cumsum([5] + [(1 << 29) - 1] * 3).tolist()
    x = np.array(top + [(1 << 31) - 1, -(1 << 31), -(1 << 31) + 3, -(1 << 31) + 2], np.int64).astype(np.int32)
    assert int(x[4]) == (1 << 31) - 1 and int(x[5]) == -(1 << 31)
    check([trace_dict(x)], 128, encoding, ">")
    # tails: fewer differences remain than the option that would otherwise fit them
    tails = [trace_dict(np.arange(n, dtype=np.int32) % 3, k) for k, n in enumerate(range(1, 16))]
    for r in range(1, 8):  # the same behind a chunk's worth of other words
        x = walk(L - 4, rng, encoding - 9)
        tails.append(trace_dict(np.concatenate([x, np.full(r, x[-1])]).astype(np.int32), 20 + r))
    check(tails, 128, encoding, ">")


@pytest.mark.parametrize("encoding", [11, 10])
def test_several_traces_in_one_call(encoding):
    """No look-ahead across a trace's end, every trace's first difference taken from 0, sequence numbers through the file."""
    rng = np.random.default_rng(3)
    dicts = [trace_dict(rng.integers(0, 4, n).astype(np.int32), k, start_us=T0 + k * 1_000_000) for k, n in enumerate((1, 7, L + 1, 5))]
    for reclen, bo in ((128, ">"), (512, "<")):
        check(dicts, reclen, encoding, bo)
    # starts off the 100 us grid: blockette 1001 on every record
    off = [trace_dict(d["data"], k, start_us=T0 + 56 + k) for k, d in enumerate(dicts)]
    st = stream_of(off)
    assert_same_file(write_mseed(st, reclen=128, encoding=encoding), OM.write_mseed(off, reclen=128, encoding=encoding, with_b1001=True), 128)


def test_settings_that_change_within_a_stream():
    """Traces of different sample types go through one call per run of equal settings; the sequence numbers go on."""
    rng = np.random.default_rng(4)
    a, b = trace_dict(walk(700, rng, 2), 0), trace_dict(rng.standard_normal(100).astype(np.float32), 1)
    c = trace_dict(walk(50, rng, 2), 2)
    got = write_mseed(stream_of([a, b, c]), reclen=128)
    want = OM.write_mseed([a], reclen=128, encoding=11)
    want += OM.write_mseed([b], reclen=128, encoding=4, seq0=1 + len(want) // 128)
    want += OM.write_mseed([c], reclen=128, encoding=11, seq0=1 + len(want) // 128)
    assert_same_file(got, want, 128)


SPECIAL_BITS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                         0x00000001, 0x807FFFFF, 0x00800000, 0x3F800000, 0xC2F6E979], np.uint32)


@pytest.mark.parametrize("byteorder", [">", "<"])
def test_plain_encodings(byteorder):
    rng = np.random.default_rng(5)
    reclen = 128
    for encoding, dtype, per in ((1, np.int32, 32), (1, np.int16, 32), (3, np.int32, 16), (4, np.float32, 16), (5, np.float64, 8)):
        for n in (3 * per, 3 * per + 1, 1):  # the last record exactly full, one sample more, one sample
            if dtype == np.float32:
                x = np.resize(SPECIAL_BITS, n).view(np.float32)
            elif dtype == np.float64:
                x = rng.standard_normal(n)
                x[:4] = [np.nan, -0.0, np.inf, 5e-324][:min(4, n)]
            else:
                x = rng.integers(-32768, 32768, n).astype(dtype)
                x[:2] = [-32768, 32767][:min(2, n)]
            dicts = [trace_dict(x, 0), trace_dict(x[::-1].copy(), 1)]
            got = write_mseed(stream_of(dicts, device=dtype != np.int16), reclen=reclen, encoding=encoding, byteorder=byteorder)
            assert_same_file(got, OM.write_mseed(dicts, reclen=reclen, encoding=encoding, byteorder=byteorder), reclen)
            back = read(got)
            assert len(back) == 2 and back[0].stats.mseed["encoding"] == encoding and back[0].stats.mseed["byteorder"] == byteorder
            if dtype == np.float32:  # NaN payloads, infinities, -0.0 and denormals come back bit for bit
                assert (back[0].data.view(np.uint32) == x.view(np.uint32)).all() and back[0].data.dtype == np.float32
            elif dtype != np.float64:
                assert (back[0].data == x).all()
    assert write_mseed(stream_of([trace_dict(np.arange(40, dtype=np.int32))]), reclen=128, encoding=3) == \
        write_mseed(stream_of([trace_dict(np.arange(40, dtype=np.int32))], device=False), reclen=128, encoding=3)


def test_refusals_name_trace_and_sample(tmp_path):
    rng = np.random.default_rng(6)
    d = np.diff(walk(2 * L + 100, rng, 2), prepend=0).astype(np.int64)
    at = L + L // 2
    bad = d.copy()
    bad[at] = 1 << 29  # one difference of 2^29 in the middle of the second chunk
    x = np.cumsum(bad).astype(np.int32)
    good = trace_dict(walk(300, rng, 2), 0)
    target = tmp_path / "never.mseed"
    for dicts in ([trace_dict(x, 1)], [good, trace_dict(x, 1)]):
        with pytest.raises(ValueError, match=rf"XX\.VOLC\.\.H01: sample {at} .*30 bits") as e:
            write_mseed(stream_of(dicts), target, reclen=512, encoding=11)
        assert "nothing was written" in str(e.value)
    assert_same_file(write_mseed(stream_of([trace_dict(x, 1)]), reclen=512, encoding=10),
                     OM.write_mseed([trace_dict(x, 1)], reclen=512, encoding=10), 512)  # Steim-1 holds it
    # two offenders: the lower index, on every run
    bad = d.copy()
    bad[L - 1], bad[3 * L // 2 + 700] = -(1 << 30), 1 << 30
    y = np.cumsum(bad).astype(np.int32)
    for _ in range(2):
        with pytest.raises(ValueError, match=rf"H01: sample {L - 1} "):
            write_mseed(stream_of([trace_dict(y, 1)]), target)
    # two traces with offenders: the first trace's
    with pytest.raises(ValueError, match=rf"H02: sample {at} "):
        write_mseed(stream_of([good, trace_dict(x, 2), trace_dict(y, 1)]), target)
    # int32 samples beyond int16 under encoding 1
    z = rng.integers(-32768, 32768, 500).astype(np.int32)
    z[[77, 401]] = [32768, -32769]
    for _ in range(2):
        with pytest.raises(ValueError, match=r"XX\.VOLC\.\.H03: sample 77 does not fit int16"):
            write_mseed(stream_of([good, trace_dict(z, 3)]), target, encoding=1, reclen=128)
    assert not target.exists()
    buf = io.BytesIO()
    with pytest.raises(ValueError):
        write_mseed(stream_of([trace_dict(z, 3)]), buf, encoding=1)
    assert buf.getvalue() == b""
    # the one deviation from a strict packer: a first sample beyond 30 bits is written, its difference stored as 0
    w = walk(L + 9, rng, 2)
    w += (1 << 30) - w[0]
    assert int(w[0]) == 1 << 30
    got = write_mseed(stream_of([trace_dict(w, 4)]), reclen=512, encoding=11)
    assert (read(got)[0].data == w).all()
    assert (OM.read_mseed(got)[0]["data"] == w).all() and got[68:72] == (1 << 30).to_bytes(4, "big")
    first_word = int.from_bytes(got[76:80], "big")  # 1 x 30 bits, or several fields of which the first is the 0
    assert first_word >> 30 != 1 or first_word & ((1 << 30) - 1) == 0


def test_round_trip_through_read():
    rng = np.random.default_rng(7)
    n = 200_000 + 123
    dicts = [dict(network="XX", station="VOLC", location="00", channel="HH" + c, start_us=T0, rate=100.0, data=walk(n, rng, 2)) for c in "ENZ"]
    dicts += [dict(network="YY", station="ETNA", location="", channel="EH" + c, start_us=T0 + 3_500_000, rate=62.5,
                   data=walk(70_001, rng, 2)) for c in "NZ"]
    st = stream_of(dicts)
    for reclen, encoding, byteorder in ((512, 11, ">"), (4096, 10, "<")):
        got = write_mseed(st, reclen=reclen, encoding=encoding, byteorder=byteorder)
        buf = io.BytesIO()
        reported = st.write(buf, format="MSEED", reclen=reclen, encoding=encoding, byteorder=byteorder)
        assert buf.getvalue() == got and reported == len(got) // reclen
        assert all(tr._data is None for tr in st)
        back = read(got, device_resident=True)
        assert [tr.id for tr in back] == sorted(tr.id for tr in st) and len(back) == len(st)
        records = 0
        for tr, src in zip(back, sorted(st, key=lambda t: t.id)):
            assert tr.id == src.id and tr.stats.starttime == src.stats.starttime and tr.stats.sampling_rate == src.stats.sampling_rate
            assert tr.stats.npts == src.stats.npts and torch.equal(tr._dev, src._dev)
            m = tr.stats.mseed
            assert (m["encoding"], m["byteorder"], m["record_length"], m["dataquality"]) == (encoding, byteorder, reclen, "D")
            assert m["steim_integrity_errors"] == 0
            records += m["number_of_records"]
        assert records == reported
        # what read() recorded is what the next write uses
        assert write_mseed(back) == write_mseed(Stream(sorted(st, key=lambda t: t.id)), reclen=reclen, encoding=encoding, byteorder=byteorder)
    assert write_mseed(stream_of(dicts, device=False), reclen=512) == write_mseed(st, reclen=512)  # host traces: the same kernels


def test_public_calls(tmp_path):
    rng = np.random.default_rng(8)
    dicts = [trace_dict(walk(3 * L, rng, 2), k, start_us=T0) for k in range(2)]
    st = stream_of(dicts)
    want = OM.write_mseed(dicts, reclen=4096, encoding=11)
    path = tmp_path / "a.mseed"
    assert st.write(path) == len(want) // 4096 and path.read_bytes() == want
    with open(tmp_path / "b.mseed", "wb") as f:
        assert st[1].write(f, reclen=512) == len(OM.write_mseed(dicts[1:], reclen=512)) // 512
    assert (tmp_path / "b.mseed").read_bytes() == OM.write_mseed(dicts[1:], reclen=512)
    with pytest.raises(ValueError, match="unsupported output format"):
        st.write(tmp_path / "c.sac", format="SAC")
    assert not (tmp_path / "c.sac").exists()
    # the scratch is kept, freed on request, and allocated again by the next write
    assert VIO.release_encode_scratch() > 0 and VIO.release_encode_scratch() == 0
    assert write_mseed(st) == want
    # a trimmed device trace is a view that does not start at its tensor's base
    tr = st[0]
    tr.trim(tr.stats.starttime + 10.07, tr.stats.starttime + 40.0)
    assert tr._dev.storage_offset() == 1007 and tr.stats.npts == 2994 and tr._data is None
    cut = trace_dict(dicts[0]["data"][1007:1007 + 2994], 0, start_us=T0 + 10_070_000)
    assert_same_file(write_mseed(tr, reclen=512), OM.write_mseed([cut], reclen=512), 512)
    assert (read(write_mseed(st, reclen=512))[0].data == cut["data"]).all()


def test_bench_entry_times_every_stage(lib):
    x = torch.from_numpy(walk(5 * L + 17, np.random.default_rng(9), 2)).cuda()
    t = _lib.VpMseedTrace()
    t.start_us, t.sample_rate, t.first_sample, t.nsamples, t.quality = T0, 100.0, 0, x.shape[0], ord("D")
    t.network, t.station, t.channel = b"XX", b"VOLC", b"HHZ"
    ms = (C.c_float * _lib.VP_MSEED_ENCODE_STAGES)()
    torch.cuda.synchronize()
    _lib.check(lib.vp_mseed_encode_bench(0, C.c_void_p(x.data_ptr()), _lib.VP_SAMPLES_INT32, C.byref(t), 1, 512, 11, 1, 3, ms))
    assert all(v > 0 for v in ms[:5]) and ms[5] == 0
    _lib.check(lib.vp_mseed_encode_bench(0, C.c_void_p(x.data_ptr()), _lib.VP_SAMPLES_INT32, C.byref(t), 1, 512, 3, 1, 3, ms))
    assert all(v == 0 for v in ms[:5]) and ms[5] > 0
    # the bench left the scratch as a write leaves it
    d = trace_dict(x.cpu().numpy())
    assert write_mseed(stream_of([d]), reclen=512) == OM.write_mseed([d], reclen=512)
