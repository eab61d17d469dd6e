"""The teeth of the bars the device STA/LTA is held to (tests/stalta_f64.py) and the host side of volpick_amd/trigger.py: no GPU.

1. the float64 restatements of the rule meet their bars against the extended-precision truth -- except the whole-trace
cumulative sum on the loud-then-quiet trace, which must miss; 2. the float64 emulation of the kernel's scheme meets them at
every seam length and window pair, and misses them with either carry broken; 3. the known answers; 4. the host paths of
``trigger.py`` equal the restatements bit for bit (classic) or within the recursive bar (``lfilter``); 5. ``Trace.trigger`` on
host traces with the reference's clipping, argument errors, ``trigger_onset`` on numpy input against tests/trigger_cases.py's
restatement; 6. the new symbols are declared, exported and bound; 7. the host header's power table and argument checks, built
into a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import volpick_amd as va
from oracle import pipeline as OP
from tests import stalta_f64 as S
from tests import trigger_cases as TC
from volpick_amd import _lib, trigger as TR

ROOT = Path(__file__).resolve().parents[1]
N = 40_003
SMALL = ((5, 20), (50, 1000), (500, 2000))


@pytest.mark.parametrize("name", list(S.INPUTS))
def test_restatements_against_the_truth(name):
    x = S.INPUTS[name](N)
    for nsta, nlta in SMALL:
        r = S.ratio("recursive", S.recursive64(x, nsta, nlta), S.truth("recursive", name, N, nsta, nlta), nsta, nlta)
        c = S.ratio("classic", S.classic64(x, nsta, nlta), S.truth("classic", name, N, nsta, nlta), nsta, nlta)
        print(f"{name} {nsta}/{nlta}: recursive loop {r:.4f} of its bar, cumulative sum {c:.4g} of the classic bar")
        assert r <= 0.07 + 1e-3
        if name == "plain":
            assert c <= 1.0
        else:
            assert c > 100.0  # the running sum has swallowed the quiet samples: not the yardstick here


def test_whole_trace_sum_bound_on_the_loud_then_quiet_trace():
    """The figure the scheme was chosen on: behind the loud samples the running sum's own rounding bound is hundreds of times
    the window it should give."""
    x = S.loud_then_quiet(N)
    worst = float(S.cumsum_bound(x, 5, 20)[20:].max())
    print(f"whole-trace sum, 5/20: rounding bound up to {worst:.0f} x the value")
    assert worst > 100.0


@pytest.mark.parametrize("nsta,nlta", S.WINDOWS)
def test_emulation_meets_the_bars_at_every_seam(nsta, nlta):
    for n in S.seam_lengths(nlta):
        x = S.plain(n)
        for kind, emu in (("classic", S.emulate_classic), ("recursive", S.emulate_recursive)):
            r = S.ratio(kind, emu(x, nsta, nlta), S.truth(kind, "plain", n, nsta, nlta), nsta, nlta)
            assert r <= 1.0, (kind, n, r)


def test_emulation_on_both_inputs_and_with_broken_carries():
    for name in S.INPUTS:
        x = S.INPUTS[name](N)
        for nsta, nlta in SMALL:
            for kind, emu in (("classic", S.emulate_classic), ("recursive", S.emulate_recursive)):
                t = S.truth(kind, name, N, nsta, nlta)
                r = S.ratio(kind, emu(x, nsta, nlta), t, nsta, nlta)
                r_tile = S.ratio(kind, emu(x, nsta, nlta, carry="no_tile"), t, nsta, nlta)
                r_piece = S.ratio(kind, emu(x, nsta, nlta, carry="no_piece"), t, nsta, nlta)
                print(f"{name} {kind} {nsta}/{nlta}: {r:.4f} of the bar; no tile carry {r_tile:.3g}, no piece carry {r_piece:.3g}")
                assert r <= 1.0 and r_tile > 1.0 and r_piece > 1.0


def test_known_answers():
    for nsta, nlta in SMALL:
        lead = nlta + 37
        x = S.zeros_then_noise(lead + 500, lead)
        for f in (S.classic64, S.emulate_classic, TR.classic_sta_lta):
            y = f(x, nsta, nlta)
            assert not y[:lead].any()
            assert abs(y[lead] - nlta / nsta) <= (nsta + nlta + 8) * S.U * nlta / nsta
        for f in (S.recursive64, S.emulate_recursive, TR.recursive_sta_lta):
            assert not f(x, nsta, nlta)[:lead].any()
        z = np.zeros(3 * nlta + 5000)  # tiny (1 - clta)^i leaves the doubles inside it
        for f in (S.classic64, S.recursive64, S.emulate_classic, S.emulate_recursive, TR.classic_sta_lta, TR.recursive_sta_lta):
            y = f(z, nsta, nlta)
            assert y.dtype == np.float64 and y.tobytes() == z.tobytes()
        short = S.plain(nlta - 1)
        for f in (S.classic64, S.recursive64, S.emulate_classic, S.emulate_recursive, TR.classic_sta_lta, TR.recursive_sta_lta):
            assert not f(short, nsta, nlta + 1).any()  # nlta > n


def test_nan_placement_of_the_emulation():
    n, nsta, nlta = 2 * S.T + 5, 5, 20
    for at in (0, 7, S.T, n - 1):
        for bad in (np.nan, np.inf):
            x = S.plain(n).copy()
            x[at] = bad
            c, r = S.emulate_classic(x, nsta, nlta), S.emulate_recursive(x, nsta, nlta)
            assert np.isnan(c[at:]).all() and not np.isnan(c[:at]).any()
            assert np.array_equal(c[:at], S.emulate_classic(S.plain(n), nsta, nlta)[:at])
            if at == 0:  # sample 0 never enters the recursion's sums, whatever it holds
                assert np.array_equal(r, S.emulate_recursive(S.plain(n), nsta, nlta))
                assert np.array_equal(S.recursive64(x, nsta, nlta), S.recursive64(S.plain(n), nsta, nlta))
                continue
            first = max(at, nlta)
            assert np.isnan(r[first:]).all() and not np.isnan(r[:first]).any() and not r[:nlta].any()
            if bad is np.nan:
                assert np.array_equal(np.isnan(S.classic64(x, nsta, nlta)), np.isnan(c))
                assert np.array_equal(np.isnan(S.recursive64(x, nsta, nlta)), np.isnan(r))


def test_host_paths_are_the_restatements():
    for name in S.INPUTS:
        x = S.INPUTS[name](N)
        for nsta, nlta in SMALL:
            for src in (x, x.astype(np.float32), x.astype(np.int64)):
                want = np.asarray(src, dtype=np.float64)
                assert TR.classic_sta_lta(src, nsta, nlta).tobytes() == S.classic64(want, nsta, nlta).tobytes()
            y = TR.recursive_sta_lta(x, nsta, nlta)
            r = S.ratio("recursive", y, S.truth("recursive", name, N, nsta, nlta), nsta, nlta)
            assert y.dtype == np.float64 and r <= 1.0
    assert TR.recursive_sta_lta(np.zeros(0), 1, 1).shape == (0,) and TR.classic_sta_lta(np.zeros(0), 1, 1).shape == (0,)
    assert TR.recursive_sta_lta(np.ones(1), 1, 1).tolist() == [0.0]
    assert va.classic_sta_lta is TR.classic_sta_lta and va.recursive_sta_lta is TR.recursive_sta_lta
    assert va.trigger_onset is TR.trigger_onset and va.sta_lta_triggers is TR.sta_lta_triggers
    assert va.release_trigger_scratch is TR.release_trigger_scratch


def test_trace_trigger_on_host_traces(lib):
    x = S.plain(5003)
    hdr = dict(network="XX", station="A", channel="HHZ", sampling_rate=100.0)
    tr = va.Trace(x.astype(np.int32), hdr)
    assert tr.trigger("recstalta", sta=5.0, lta=20.0) is tr
    assert tr.data.dtype == np.float64 and tr.stats.npts == 5003
    assert np.array_equal(tr.data, TR.recursive_sta_lta(x, 500, 2000))
    tr = va.Trace(x, hdr)
    tr.trigger("classicstalta", sta=0.05, lta=0.2)
    assert np.array_equal(tr.data, S.classic64(x, 5, 20))
    # the reference's clipping: min(int(lta * sr), n), and never below one sample
    tr = va.Trace(x, hdr)
    tr.trigger("recstalta", sta=5.0, lta=200.0)
    assert np.array_equal(tr.data, TR.recursive_sta_lta(x, 500, 5003)) and not tr.data.any()
    tr = va.Trace(x, hdr)
    tr.trigger("classicstalta", sta=0.001, lta=0.2)
    assert np.array_equal(tr.data, S.classic64(x, 1, 20))
    st = va.Stream([va.Trace(x, hdr), va.Trace(x[:3000], dict(hdr, channel="HHN"))])
    assert st.trigger("recstalta", sta=1.0, lta=4.0) is st
    assert np.array_equal(st[1].data, TR.recursive_sta_lta(x[:3000], 100, 400))
    # the reference's check in one call, host traces: triggers cut from the float32 cft by the host mirror
    x = S.bursts(5003)
    st = va.Stream([va.Trace(x, hdr), va.Trace(x[:3000], dict(hdr, channel="HHN"))])
    res = va.sta_lta_triggers(st, sta=0.05, lta=0.2)  # the reference's thresholds: 2 and 0.5
    assert set(res) == {"XX.A..HHZ", "XX.A..HHN"} and st[0].data is x
    for tr_ in st:
        got = res[tr_.id]
        cft = TR.recursive_sta_lta(tr_.data, 5, 20)
        assert np.array_equal(got["cft"], cft)
        want = OP.picks_from_trace(cft.astype(np.float32), 2.0, 0.5)
        assert len(want) > 3
        TC.same(list(zip(got["on"], got["off"], got["peak"], got["value"])), want)


@pytest.mark.parametrize("case", S.TRIGGER_CASES)
def test_trigger_cases_stand_clear_of_their_thresholds(case):
    kind, n, nsta, nlta, thr_on, thr_off = case
    S.clear_of_thresholds(kind, S.truth(kind, "bursts", n, nsta, nlta), nsta, nlta, thr_on, thr_off)


def test_argument_errors(lib):
    x = S.plain(100)
    for f in (TR.classic_sta_lta, TR.recursive_sta_lta):
        for nsta, nlta in ((0, 5), (6, 5), (-1, -1)):
            with pytest.raises(ValueError, match="nsta <= nlta"):
                f(x, nsta, nlta)
        with pytest.raises(ValueError, match="1-D"):
            f(np.zeros((2, 50)), 1, 2)
        with pytest.raises(NotImplementedError, match="split the stream at its gaps first"):
            f(np.ma.masked_array(x, mask=x > 123456), 1, 2)
    hdr = dict(network="XX", station="A", channel="HHZ", sampling_rate=100.0)
    with pytest.raises(ValueError, match="not one of"):
        va.Trace(x, hdr).trigger("zdetect", sta=1, lta=2)
    with pytest.raises(ValueError, match="longer than"):
        va.Trace(x, hdr).trigger("recstalta", sta=0.5, lta=0.2)
    with pytest.raises(ValueError, match="not one of"):
        va.sta_lta_triggers(va.Stream([va.Trace(x, hdr)]), type="carlstatrig")
    with pytest.raises(NotImplementedError, match="max_len"):
        TR.trigger_onset(x, 2.0, 0.5, max_len=100)
    with pytest.raises(ValueError, match="one series"):
        TR.trigger_onset(np.zeros((2, 5)), 2.0, 0.5)


def test_trigger_onset_on_numpy_input(lib):
    checked = 0
    for c in TC.all_cases():
        for pair in c.pairs:
            want = TC.expected()[(c.name, pair)]
            got = TR.trigger_onset(c.x, *pair)
            assert got.dtype == np.int64 and got.shape == (len(want), 2)
            assert got.tolist() == [[int(w[0]), int(w[1])] for w in want], (c.name, pair)
            checked += 1
    assert checked > 500
    assert TR.trigger_onset(np.zeros(0, np.float32), 2.0, 0.5).shape == (0, 2)
    z = np.load(ROOT / "tests" / "golden" / "trigger_cases.npz")
    assert len(TR.trigger_onset(z["x"], 0.3, 0.3)) > 0
    # thr2 > thr1: the general rule is the host path's
    x = np.array([0, 1, 0, 3, 3, 0], np.float32)
    assert TR.trigger_onset(x, 0.5, 2.0).tolist() == [[1, 4]]


def test_symbols_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "volpick_hip.h").read_text()
    for name in ("vp_sta_lta", "vp_sta_lta_release_scratch", "vp_sta_lta_bench", "vp_trigger_onset"):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, f"{name} is not declared in volpick_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"enum \{ VP_STALTA_CLASSIC = 0, VP_STALTA_RECURSIVE = 1 \};", header)
    assert (_lib.VP_STALTA_CLASSIC, _lib.VP_STALTA_RECURSIVE) == (0, 1)
    host_h = (ROOT / "volpick_amd" / "csrc" / "stalta_host.h").read_text()
    assert f"STALTA_MAX_NLTA = {S.MAX_NLTA};" in host_h and f"STALTA_PIECE = {S.P};" in host_h
    # refused without a device: nothing is touched
    out = np.full(8, -77.0, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.vp_sta_lta(0, p, 1, 1, 8, 8, 1, 0, 5, p, 1) == -1 and b"vp_sta_lta" in lib.vp_last_error()
    assert lib.vp_sta_lta(0, None, 1, 1, 8, 8, 1, 1, 5, p, 1) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_sta_lta(0, None, 1, 1, 8, 8, 1, 1, S.MAX_NLTA + 1, p, 1) == -1
    n = C.c_int(5)
    assert lib.vp_trigger_onset(0, p, 1, 8, 8, 0.5, 2.0, None, None, None, None, None, 0, 0, C.byref(n)) == -1
    assert b"vp_pick_host" in lib.vp_last_error() and (out == -77.0).all()


def test_host_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/llvm/bin/clang++")
    exe = tmp_path / "stalta_host_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-I", str(ROOT / "volpick_amd" / "csrc"),
           str(ROOT / "tests" / "stalta_host_check.cpp"), "-o", str(exe)]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + sanitize, capture_output=True).returncode != 0:  # no sanitizer runtime for this compiler
        print("sanitizer build failed; building without")
        subprocess.run(cmd, check=True)
    pairs = list(S.WINDOWS) + [(1, 2), (2, 2), (20, S.MAX_NLTA)]
    r = subprocess.run([str(exe)] + [str(v) for pr in pairs for v in pr], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    lines = r.stdout.splitlines()
    L = np.longdouble
    for k, (nsta, nlta) in enumerate(pairs):
        assert lines[3 * k] == f"table {nsta} {nlta}"
        for s, w in enumerate((nsta, nlta)):
            v = [float.fromhex(t) for t in lines[3 * k + 1 + s].split()]
            assert len(v) == 18 and v[0] == 1.0 / w and v[1] == 1.0 - 1.0 / w
            for lev in range(16):
                want = L(v[1]) ** (S.P * 2 ** lev)
                # one rounding to double on a power that is right to about 2^(lev + 5) 2^-64; a power under the doubles is 0
                assert abs(L(v[2 + lev]) - want) <= (2.0 ** -53 + 2.0 ** (lev + 6 - 64)) * want + 5e-324, (nsta, nlta, lev)
    codes = dict(ln.split()[1:] for ln in lines[3 * len(pairs):])
    assert len(codes) == 17
    for name, code in codes.items():
        want = 0 if name.startswith("valid") else (-4 if name == "nlta_beyond_limit" else -1)
        assert int(code) == want, name
