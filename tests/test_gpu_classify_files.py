"""``model.classify_files(sources)`` against the loop it stands for,
``[model.classify(read(s, device_resident=True)) for s in sources]``: the station blocks the one-launch decode writes are the
assembly's bit for bit, the picks and detections are the same records with the same ``peak_value`` bits whichever route a file
takes, and the pipeline keeps files, ring slots and threads apart."""
import struct
import threading
import warnings

import numpy as np
import pytest

import volpick_amd.io as vio
from oracle import mseed as OM
from tests.files_util import as_encoding, layout_bytes, layouts, log_channel_bytes, trace
from tests.mseed_util import T0, file_bytes
from volpick_amd import _lib, pinned_array
from volpick_amd.synthetic import synthetic_stream_array

pytestmark = pytest.mark.gpu

PN_README = dict(overlap=2500, blinding=(250, 250), stacking="max", P_threshold=0.2, S_threshold=0.25)
EQT_README = dict(batch_size=256, overlap=5500, blinding=(500, 500), stacking="avg", P_threshold=0.2, S_threshold=0.2)


# ------------------------------------------------------------------------------------------ block bits
_STREAM = [None]  # one stream for every decode of this module


def decoded_blocks(buf, order="ZNE", rate=100.0, in_samples=3001):
    """(blocks the new entry writes through the plan, its status per record, the table)."""
    import torch

    from volpick_amd.files import decode_plan, plan_groups

    table, seg = vio.scan_segments(buf)
    plan = vio.plan_file_blocks(table, seg, order, rate, in_samples, warn=False)
    assert plan.reason is None
    image = torch.from_numpy(np.frombuffer(buf + b"\0" * 8, np.uint8).copy()).cuda()
    table_host = pinned_array(len(table) * _lib.VP_MSEED_TABLE_BYTES_PER_RECORD, np.uint8)
    table_dev = torch.empty(table_host.size, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    stream = _STREAM[0] = _STREAM[0] or torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rc, out, status = decode_plan(torch, 0, image, len(buf), table, plan, table_host, table_dev, stream)
        _lib.check(rc, "vp_mseed_decode_on")
        status = status.cpu().numpy()
    return plan_groups(plan, out), status, table


def assembled_blocks(buf, order="ZNE", rate=100.0, in_samples=3001):
    """(_group_stream's blocks of read(buf, device_resident=True), vp_mseed_decode's status per record)."""
    from volpick_amd.models import _group_stream

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        groups = list(_group_stream(vio.read(buf, device_resident=True), order, rate, True, in_samples))
    r, seg = vio._segments(vio.scan_mseed(buf))
    _, buffers = vio._decode(buf, r, (0, len(r)), (0,), 0, None, True)
    return groups, sum(status for _, _, status in buffers.values())


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def assert_blocks_equal(buf):
    got, status, table = decoded_blocks(buf)
    want, want_status = assembled_blocks(buf)
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        a, b = host(g["data"]), host(w["data"])
        assert isinstance(g["data"], np.ndarray) == isinstance(w["data"], np.ndarray)  # zeros nothing feeds stay on the host
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert (g["trace_id"], g["starttime"]._us) == (w["trace_id"], w["starttime"]._us)
    assert np.array_equal(status, want_status)
    return status


def steim_mismatch(buf, reclen, record=2):
    """The file with the reverse integration constant of one record off by one."""
    b = bytearray(buf)
    b[record * reclen + 64 + 11] ^= 1
    return bytes(b)


@pytest.mark.parametrize("reclen", [256, 512, 4096])
@pytest.mark.parametrize("byteorder", ["<", ">"])
@pytest.mark.parametrize("encoding", [1, 3, 4, 5, 10, 11])
def test_block_bits_mseed2(lib, encoding, byteorder, reclen):
    for name, traces in layouts().items():
        buf = layout_bytes(as_encoding(traces, encoding), reclen=reclen, encoding=encoding, byteorder=byteorder)
        if name == "three_components":
            buf += log_channel_bytes(4000, reclen)
        status = assert_blocks_equal(buf)
        assert not status.any()
        if encoding in (10, 11) and name == "late_start_early_end":
            status = assert_blocks_equal(steim_mismatch(buf, reclen))
            assert sorted(status)[-2:] == [0, 1]


@pytest.mark.parametrize("encoding", [1, 3, 4, 5, 10, 11])
def test_block_bits_mseed3(lib, encoding):
    for name, traces in layouts().items():
        buf = layout_bytes(as_encoding(traces, encoding), version=3, encoding=encoding, max_payload=448 if name < "m" else 1472,
                           extra_headers=b'{"a":1}' if name > "m" else b"")
        assert not assert_blocks_equal(buf).any()


# ------------------------------------------------------------------------------------------ equal results
def plain(out):
    us = lambda t: None if t is None else int(t._us)  # noqa: E731
    bits = lambda v: struct.pack("<d", float(v))  # noqa: E731
    picks = [(p.trace_id, p.phase, us(p.start_time), us(p.end_time), us(p.peak_time), bits(p.peak_value)) for p in out.picks]
    dets = [(q.trace_id, us(q.start_time), us(q.end_time), bits(q.peak_value)) for q in (getattr(out, "detections", None) or [])]
    return picks, dets


def loop(model, sources, **kw):
    """The per-file loop, with the warnings of each file."""
    outs, warned = [], []
    for s in sources:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            outs.append(plain(model.classify(vio.read(s, device_resident=True), **kw)))
        warned += [str(x.message) for x in w]
    return outs, warned


def pipelined(model, sources, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        outs = [plain(o) for o in model.classify_files(sources, **kw)]
    return outs, [str(x.message) for x in w]


def event_traces(n, seed, sta="VOLC", rate=100.0, first=0, channels=("HHZ", "HHN", "HHE")):
    """Three components with P and S arrivals, as integer counts."""
    data, _, _ = synthetic_stream_array(n, seed=seed, n_events=max(2, n // 3000))
    return [trace(c, n, first, sta=sta, rate=rate, data=np.round(data[i] * 4000).astype(np.int32))
            for i, c in enumerate(channels)]


def zero_sample_file():
    buf = bytearray(file_bytes([trace("HHZ", 100, data=np.arange(100))]))
    buf[30:32] = b"\0\0"
    return bytes(buf[:512])


def sac_file(n=8001, seed=77):
    data, _, _ = synthetic_stream_array(n, seed=seed, n_events=3)
    return OM.write_sac(data[0].astype(np.float32), 100.0, T0, "XX", "SACS", "", "HHZ")


def varied_files(n, seed):
    """Files that between them take every way through the call: planned blocks (full, zero-filled, two per file, host zeros
    beside data), and each kind of file the plan leaves to read()."""
    ev = lambda m, k, **kw: event_traces(m, seed + k, **kw)  # noqa: E731
    late = ev(n, 2)
    late[1] = dict(late[1], start_us=late[1]["start_us"] + 5_004_900, data=late[1]["data"][:n - 1500])
    two = ev(n, 3) + ev(n - 500, 4, first=n + 900)
    return {
        "plain": file_bytes(ev(n, 1)),
        "late start, early end": file_bytes(late, reclen=4096),
        "two blocks, mseed3": OM.write_mseed3(two),
        "two instruments and a LOG channel": file_bytes(ev(n, 5) + ev(n + 40, 6, sta="OTHR")[:2]) + log_channel_bytes(4000),
        "50 Hz": file_bytes(ev(n, 7, rate=50.0)),
        "same-component overlap": file_bytes(ev(n, 8) + [trace("HHZ", 3500, 3000, np.random.default_rng(seed))]),
        "SAC": sac_file(n),
        "only a short run": file_bytes(ev(2000, 9)),
        "no records": zero_sample_file(),
    }


@pytest.fixture(scope="module")
def phasenet(lib):
    from volpick_amd import PhaseNet

    return PhaseNet.from_pretrained("volpick").cuda()


@pytest.fixture(scope="module")
def eqt(lib):
    from volpick_amd import EQTransformer

    return EQTransformer.from_pretrained("volpick").cuda()


def assert_same_as_loop(model, sources, min_picks=1, depth=2, workers=2, **kw):
    want, want_warned = loop(model, sources, **kw)
    got, got_warned = pipelined(model, sources, depth=depth, workers=workers, **kw)
    assert len(got) == len(want) == len(sources)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"file {k}"
    assert sorted(got_warned) == sorted(want_warned)
    assert sum(len(w[0]) + len(w[1]) for w in want) >= min_picks  # picks and detections
    return want, want_warned


@pytest.mark.parametrize("kw", [{}, PN_README], ids=["defaults", "README arguments"])
def test_phasenet_files_equal_the_loop(phasenet, kw):
    files = varied_files(9001, 100)
    want, warned = assert_same_as_loop(phasenet, list(files.values()), **kw)
    names = list(files)
    assert want[names.index("only a short run")] == ([], []) and want[names.index("no records")] == ([], [])
    assert sum("fragments shorter than the number of input samples" in w for w in warned) == 1
    # which files the plan kept and which it left to read()
    stats = {}
    pipelined(phasenet, list(files.values()), _stats=stats, **kw)
    assert stats["fallback_files"] == 4  # 50 Hz, overlap, SAC, and the record-less file


def test_phasenet_long_route_and_single_blocks(phasenet):
    """batch_size=1 makes a 12001-sample block 'long' (six windows on three contexts): the segment route, fed by planned
    blocks; one file then holds a long and a short block."""
    n = 12001
    assert phasenet._is_long(n, phasenet._argdict(dict(batch_size=1)))
    files = [file_bytes(event_traces(n, 201)), file_bytes(event_traces(n, 202) + event_traces(7001, 203, first=n + 700)),
             file_bytes(event_traces(7001, 204))]
    assert_same_as_loop(phasenet, files, batch_size=1)


def test_phasenet_model_with_a_filter_takes_the_existing_route(lib):
    from volpick_amd import PhaseNet

    base = PhaseNet.from_pretrained("volpick")
    model = PhaseNet(norm=base.norm, component_order=base.component_order, phases=base.labels, filter_args=("highpass",),
                     filter_kwargs={"freq": 0.5})
    model.load_state_dict(base.state_dict())
    model.default_args = dict(base.default_args)
    model.cuda()
    files = [file_bytes(event_traces(8001, 301 + k)) for k in range(3)]
    stats = {}
    assert_same_as_loop(model, files)
    model.classify_files(files, _stats=stats)
    assert stats["fallback_files"] == 3


@pytest.mark.parametrize("kw", [{}, EQT_README, dict(EQT_README, stacking="max", batch_size=1)],
                         ids=["defaults", "README arguments", "long route"])
def test_eqtransformer_files_equal_the_loop(eqt, kw):
    n = 13001
    if kw.get("batch_size") == 1:
        assert eqt._is_long(n, eqt._argdict(kw))
    files = [file_bytes(event_traces(n, 401)), OM.write_mseed3(event_traces(n, 402, channels=("HH3", "HH1", "HH2"))),
             file_bytes(event_traces(n, 403)[:2], reclen=4096), file_bytes(event_traces(n, 404, rate=50.0))]
    assert_same_as_loop(eqt, files, **kw)


# ------------------------------------------------------------------------------------------ the pipeline itself
def seven_files():
    return [file_bytes(event_traces(7001 if k % 2 == 0 else 28001, 500 + k)) for k in range(7)]


@pytest.fixture(scope="module")
def seven(phasenet):
    files = seven_files()
    return files, loop(phasenet, files)[0]


@pytest.mark.parametrize("depth, workers", [(1, 1), (1, 4), (2, 2), (3, 1), (3, 4), (2, 4), (1, 2), (3, 2), (2, 1)])
def test_ring_slots_reused_and_regrown(phasenet, seven, depth, workers):
    files, want = seven
    assert pipelined(phasenet, files, depth=depth, workers=workers)[0] == want


def test_outputs_follow_their_sources(phasenet, seven):
    files, want = seven
    order = [4, 1, 6, 0, 3, 5, 2]
    got = pipelined(phasenet, [files[i] for i in order])[0]
    assert got == [want[i] for i in order]
    assert len({repr(w) for w in want}) == len(want)  # (the files do differ)


def test_refused_file_in_the_middle(phasenet, seven):
    files, want = seven
    short = bytearray(file_bytes(as_encoding(event_traces(7001, 600), 3), encoding=3))
    short[3 * 512 + 30:3 * 512 + 32] = struct.pack(">H", 500)  # the fourth record claims 500 samples in 448 bytes
    short = bytes(short)
    with pytest.raises(ValueError) as per_file:
        vio.read(short, device_resident=True)
    assert "payload holds fewer samples" in str(per_file.value)
    with pytest.raises(ValueError) as e:
        phasenet.classify_files(files[:3] + [short] + files[3:])
    assert str(e.value) == str(per_file.value)
    assert pipelined(phasenet, files)[0] == want  # at once, on the same handle
    # ... and the other refusals: what read() says, from the same call
    crc = bytearray(OM.write_mseed3(event_traces(7001, 601)))
    crc[70] ^= 1
    for bad, exc in ((bytes(crc), _lib.VolpickHipError), (b"neither format", ValueError)):
        with pytest.raises(exc) as per_file:
            vio.read(bad, device_resident=True)
        with pytest.raises(exc) as e:
            phasenet.classify_files([files[0], bad, files[1]])
        assert str(e.value) == str(per_file.value)
    with pytest.raises(FileNotFoundError):
        phasenet.classify_files([files[0], "/nonexistent/volpick.mseed"])


def test_paths_and_file_objects(phasenet, seven, tmp_path):
    import io

    files, want = seven
    path = tmp_path / "a.mseed"
    path.write_bytes(files[0])
    got = pipelined(phasenet, [path, str(path), io.BytesIO(files[2]), bytearray(files[4])])[0]
    assert got == [want[0], want[0], want[2], want[4]]
    assert phasenet.classify_files([]) == []


def test_two_models_on_two_threads(phasenet, eqt, seven):
    files, want_pn = seven
    eqt_files = [file_bytes(event_traces(13001, 700 + k)) for k in range(3)]
    want_eqt = pipelined(eqt, eqt_files, **EQT_README)[0]
    assert want_eqt == loop(eqt, eqt_files, **EQT_README)[0]
    gate, results = threading.Barrier(2), {}

    def job(name, model, sources, kw):
        try:
            gate.wait(timeout=60)
            results[name] = [[plain(o) for o in model.classify_files(sources, **kw)] for _ in range(2)]
        except BaseException as e:  # noqa: BLE001
            results[name] = e

    threads = [threading.Thread(target=job, args=("pn", phasenet, files, {})),
               threading.Thread(target=job, args=("eqt", eqt, eqt_files, EQT_README))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads)
    assert results["pn"] == [want_pn, want_pn]
    assert results["eqt"] == [want_eqt, want_eqt]
