"""Station layouts and file bytes shared by the file-pipeline tests (tests/test_files_plan_cpu.py,
tests/test_gpu_classify_files.py, the file route of tests/test_group_stream_cpu.py): every way a miniSEED file's traces can sit
in their station blocks, and a block plan's cells by sample number."""
import numpy as np

import volpick_amd.io as vio
from oracle import mseed as OM
from tests.mseed_util import T0, file_bytes, seismogram

PERIOD_US = 10_000  # 100 Hz


def trace(channel, n, first=0, rng=None, sta="VOLC", net="XX", loc="", rate=100.0, shift_us=0, data=None):
    """One trace dict for the oracle's writers, ``first`` samples (and ``shift_us``) after T0."""
    if data is None:
        data = seismogram(n, rng, scale=200, spikes=False)
    return dict(network=net, station=sta, location=loc, channel=channel, start_us=T0 + first * PERIOD_US + shift_us, rate=rate,
                data=np.asarray(data))


def layouts(n=7001, seed=3):
    """{name: [trace dicts]}: the layouts the block plan has to get right, each trace ``n`` samples unless the layout is about
    its length.  (``n`` >= twice PhaseNet's 3001-sample window keeps more than one window per block.)"""
    rng = np.random.default_rng(seed)
    t = lambda cha, m=n, first=0, **kw: trace(cha, m, first, rng, **kw)  # noqa: E731
    return {
        "one_component": [t("HHZ")],
        "two_components_one_missing": [t("HHZ"), t("HHE")],
        "three_components": [t("HHZ"), t("HHN"), t("HHE")],
        # N begins 500.49 sample periods late and stops early: zero fill on both sides, and a start off the sample grid
        "late_start_early_end": [t("HHZ"), t("HHN", n - 1500, 500, shift_us=4900), t("HHE")],
        "gap_in_one_component": [t("HHZ", 3000), t("HHZ", n - 3400, 3400), t("HHN"), t("HHE")],
        "gap_splits_two_blocks": [t(c, m, first) for c in ("HHZ", "HHN", "HHE") for m, first in ((n, 0), (n - 1000, n + 800))],
        "fragment_below_window": [t(c, m, first) for c in ("HHZ", "HHN", "HHE") for m, first in ((n, 0), (2000, n + 500))],
        "names_123": [t("HH3"), t("HH1"), t("HH2")],
        "two_instruments": [t("HHZ"), t("HHN"), t("HHE"), t("EHZ", n + 13, 40), t("EHN", n + 13, 40), t("EHE", n + 13, 40),
                            t("HHZ", sta="OTHR"), t("HHE", sta="OTHR", first=7)],
    }


def layout_bytes(traces, version=2, **kw):
    """The layout as one file: miniSEED 2 (``file_bytes``' arguments) or miniSEED 3 (``write_mseed3``'s)."""
    return file_bytes(traces, **kw) if version == 2 else OM.write_mseed3(traces, **kw)


def table_layout(table, seg):
    """The segments of ``scan_segments``' table as a layout of tests/stream_restate.py, in table order: each segment's samples
    are 1 + their global sample number (0 is then a cell nothing fed), so that a block cell names the record and the offset it
    came from."""
    ns = table["nsamples"].astype(np.int64)
    base = np.cumsum(ns) - ns
    text = lambda field, a: table[field][a].decode()  # noqa: E731
    return [(text("network", a), text("station", a), text("location", a), text("channel", a), int(table["start_us"][a]),
             np.arange(base[a] + 1, base[a] + 1 + int(ns[a:b].sum()), dtype=np.float32))
            for a, b in zip(*vio._segment_ranges(seg))]


def planned_blocks(table, plan):
    """The blocks of ``io.plan_file_blocks``' plan as arrays: every record writes 1 + its global sample numbers where
    ``out_index`` sends it.  No two records may share a cell, none may land outside the blocks, no two blocks overlap."""
    ns = table["nsamples"].astype(np.int64)
    base = np.cumsum(ns) - ns
    cells, writes = np.zeros(plan.n_out, np.float32), np.zeros(plan.n_out, np.int32)
    for r in np.flatnonzero(plan.out_index >= 0):
        lo = int(plan.out_index[r])
        cells[lo:lo + ns[r]] = np.arange(base[r] + 1, base[r] + 1 + ns[r], dtype=np.float32)
        writes[lo:lo + ns[r]] += 1
    assert writes.max(initial=0) <= 1  # no two records share a cell
    out, claimed = [], np.zeros(plan.n_out, bool)
    for b in plan.blocks:
        c, n = b["shape"]
        if b["offset"] < 0:
            out.append(np.zeros((c, n), np.float32))
            continue
        assert b["offset"] % vio.BLOCK_ALIGN == 0 and not claimed[b["offset"]:b["offset"] + c * n].any()
        claimed[b["offset"]:b["offset"] + c * n] = True
        out.append(cells[b["offset"]:b["offset"] + c * n].reshape(c, n))
    assert not writes[~claimed].any()  # and none lands outside the blocks
    return out


def log_channel_bytes(n=4000, reclen=512):
    """A LOG channel as text records (encoding 0) at the data's rate: an instrument with no component row of its own."""
    text = (np.arange(n) % 64 + 32).astype(np.int32)
    return file_bytes([trace("LOG", n, data=text)], reclen=reclen, encoding=OM.ENC_TEXT)


def as_encoding(traces, encoding):
    """The traces with samples every record of ``encoding`` can hold exactly: int16 range for encoding 1, floats with a
    fraction for the float encodings (float64 ones that float32 rounds)."""
    out = []
    for tr in traces:
        d = np.asarray(tr["data"]).astype(np.int64)
        if encoding == OM.ENC_INT16:
            d = (d % 60001 - 30000).astype(np.int32)
        elif encoding == OM.ENC_FLOAT32:
            d = (d.astype(np.float32) * np.float32(0.37)).astype(np.float32)
        elif encoding == OM.ENC_FLOAT64:
            d = d.astype(np.float64) * 0.1234567890123
        else:
            d = d.astype(np.int32)
        out.append(dict(tr, data=d))
    return out
