"""The sequence of library calls behind classify() / annotate() is the parent build's, call for call.

The order in which the host path issues uploads, submits and collects over the device contexts and submit slots is what
overlaps one block's copy with another's compute.  The result tests (long against unsplit, multi against per-block, many
stations against single calls, pinned against pageable) cannot see it move.  tests/golden/classify_call_trace.json holds, for
five calls (four of classify() / annotate(), one of classify_files(), whose files take the long route, the resident route and
the way through read()), one row per vp_annotate / vp_classify_submit / vp_classify_collect / vp_classify_multi / vp_pick_rows (function,
context, slot, sample count or block lengths, number of trigger specs, capacity, overlap, blinding, stacking, batch) and
the pick lists (times in microseconds, the float32 value's bits).  It was recorded on the GPU from the commit BEFORE the
consolidation of volpick_amd/models.py with tools/record_classify_call_trace.py, which also holds the cases and the recorder:
a forwarding stand-in for the loaded library (`volpick_amd._lib._lib`), installed for the duration of the call.  The
classify_files() case was recorded from the commit before that call's loop over the blocks became classify()'s own.

What a disturbed schedule looks like: a long block's collects ahead of the next block's submits (the upload no longer runs
beside the last segments), both blocks on one set of submit slots, the block behind cut as finely as the first, short host
blocks all on context 0, a device chunk flushed a block early, the profiled mode's uploads interleaved with its submits."""
import importlib.util
import json
from pathlib import Path

import pytest

from volpick_amd import _lib

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_classify_call_trace",
                                               Path(__file__).resolve().parents[1] / "tools" / "record_classify_call_trace.py")
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


@pytest.fixture(scope="module")
def golden():
    return tool.load_golden()


def test_golden_file_holds_every_case(golden):
    assert sorted(golden) == sorted(tool.CASES)
    assert all(len(case["calls"]) > 0 for case in golden.values())


@pytest.mark.parametrize("name", list(tool.CASES))
def test_call_sequence_and_results_are_the_parent_builds(golden, monkeypatch, name):
    lib = _lib.load()
    got = tool.run_case(name, lambda rec: monkeypatch.setattr(_lib, "_lib", rec if rec is not None else lib))
    got = json.loads(json.dumps(got))  # tuples -> lists, as the file has them
    want = golden[name]
    assert sorted(got) == sorted(want)
    for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"{name}: call {i} is {dict(zip(tool.COLUMNS, a))}, the parent issued {dict(zip(tool.COLUMNS, b))}"
    assert len(got["calls"]) == len(want["calls"])
    for key in want:
        assert got[key] == want[key], f"{name}: {key}"
    if "picks" in want:
        assert len(want["picks"]) > 0


def test_the_cases_exercise_every_route(golden):
    """The recorded calls themselves: what the cases were built to reach is in the file."""
    col = {c: i for i, c in enumerate(tool.COLUMNS)}
    full = golden["phasenet_classify"]["calls"]
    submits = [r for r in full if r[0] == "classify_submit"]
    long_submits = [r for r in submits if r[col["n_specs"]] == 0]  # segments: rows out, no trigger scan
    assert {r[col["slot"]] for r in long_submits} == {0, 1, 2, 3}  # both sets of submit slots
    assert {r[col["context"]] for r in long_submits} == {0, 1, 2}
    short = [r for r in submits if r[col["n_specs"]] > 0]
    assert [r[col["context"]] for r in short[:5]] == [0, 1, 2, 0, 1] and all(r[col["slot"]] == 0 for r in short)
    multi = [r for r in full if r[0] == "classify_multi"]
    assert len(multi) == 1 and len(multi[0][col["samples"]]) == 3 and len(short) == 6  # five host blocks + the chunk of one
    assert sum(r[0] == "pick_rows" for r in full) == 4
    prof = golden["phasenet_classify_profiled"]
    assert prof["timing_keys"] == sorted(["h2d_ms", "gpu_ms", "windows", "pick_scan_d2h_ms", "emit_records_ms", "host_assembly_ms"])
    eqt = [r for r in golden["eqtransformer_classify"]["calls"] if r[0] == "classify_submit" and r[col["n_specs"]] == 0]
    assert {r[col["context"]] for r in eqt} == {0, 1, 2, 3}
    assert [r[0] for r in golden["phasenet_annotate"]["calls"]].count("annotate") == 1
    files = golden["phasenet_classify_files"]
    assert sum(r[0] == "classify_submit" and r[col["n_specs"]] == 0 for r in files["calls"]) == 6  # file 0: one long block
    assert [r[col["samples"]] for r in files["calls"] if r[0] == "classify_multi"] == [[20000, 15000], [20000, 15000, 8000]]
    assert {p[0] for p in files["picks"]} == {0, 1, 2} and any(p[1] == "XX.H2." for p in files["picks"])  # the 50 Hz trace, resampled
