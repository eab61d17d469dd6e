"""The float64 restatement of the spectrogram rule (tests/spectrogram_f64.py) against ``matplotlib.mlab.specgram`` plus the six
lines of the reference's ``spectrogram()`` behind it (volpick/data/utils.py:1342-1366), the host plan of the package
(``volpick_amd.spectrogram.plan``) against the restatement's, the teeth of the bound, and the host checks of ``vp_spectrogram``
(volpick_amd/csrc/spectrogram_host.h) driven by a stand-alone program under AddressSanitizer / UBSan.  No GPU."""
import math
import os
import re
import shutil
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import spectrogram_f64 as S

ROOT = Path(__file__).resolve().parents[1]

# name -> (npts, samp_rate, keywords): the plans tests/test_gpu_spectrogram.py runs on the device as well
PLANS = {
    "defaults, 3001 samples": (3001, 100.0, {}),
    "defaults, 141 samples (two frames)": (141, 100.0, {}),
    "wlen 2.56 s at 100 Hz (256 / 2048)": (6000, 100.0, {"wlen": 2.56}),
    "50 Hz, per_lap 0.5, mult None": (3000, 50.0, {"per_lap": 0.5, "mult": None}),
    "200 Hz, mult 1, dbscale": (4000, 200.0, {"mult": 1.0, "dbscale": True}),
    "wlen 1 s, mult 3 (becomes 2)": (3001, 100.0, {"wlen": 1.0, "mult": 3.0}),
    "per_lap 0, mult 2": (3001, 100.0, {"per_lap": 0.0, "mult": 2.0}),
}


def reference_numbers(data, samp_rate, per_lap=0.9, wlen=None, dbscale=False, mult=8.0):
    """The reference's spectrogram() from its first line to ``freq = freq[1:]``, the length checks left out (one frame is let
    through: the 128-sample plan)."""
    from matplotlib import mlab

    samp_rate = float(samp_rate)
    if not wlen:
        wlen = 128 / samp_rate
    nfft = int(S.nearest_pow_2(wlen * samp_rate))
    if mult is not None:
        mult = int(S.nearest_pow_2(mult))
        mult = mult * nfft
    nlap = int(nfft * float(per_lap))
    data = data - data.mean()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # "Only one segment is calculated": the 128-sample plan
        specgram, freq, time = mlab.specgram(data, Fs=samp_rate, NFFT=nfft, pad_to=mult, noverlap=nlap)
    with np.errstate(divide="ignore"):
        specgram = 10 * np.log10(specgram[1:, :]) if dbscale else np.sqrt(specgram[1:, :])
    return specgram, freq[1:], time


@pytest.mark.parametrize("name", list(PLANS) + ["defaults, 128 samples (one frame)"])
def test_restatement_equals_mlab_specgram_plus_the_references_six_lines(name):
    pytest.importorskip("matplotlib")
    npts, rate, kw = PLANS.get(name, (128, 100.0, {}))
    x = S.signal(npts, 21, rate)
    want, wf, wt = reference_numbers(x, rate, **kw)
    if npts == 128:  # the reference refuses one frame behind mlab.specgram; the arithmetic itself is compared here
        nfft, pad, hop = 128, 1024, 13
        amp = S._amplitudes(x, rate, nfft, pad, hop, (0, 1))
        got, (gf, gt) = amp[1:], S.axes(npts, rate, nfft, pad, hop)
        with pytest.raises(ValueError):
            S.plan(npts, rate)
    else:
        got, gf, gt, _ = S.spectrogram_f64(x, rate, **kw)
    assert got.shape == want.shape
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print(f"{name}: shape {got.shape}, max |restatement - mlab| / max |mlab| = {err:.2e}")
    assert err <= 1e-13
    assert np.array_equal(gf, wf) and np.array_equal(gt, wt)


def test_plan_of_the_package_equals_the_restatement_and_raises_where_the_reference_raises():
    from volpick_amd import spectrogram as VS

    n = 0
    for npts in (128, 140, 141, 142, 255, 256, 1000, 3001, 6000, 100_003):
        for rate in (20.0, 50.0, 100.0, 200.0, 250.0):
            for per_lap in (0.0, 0.5, 0.9, 0.99):
                for wlen in (None, 0.32, 1.0, 1.92, 2.56, 3.84):  # 1.92 s and 3.84 s at 100 Hz: ties, which go down
                    for mult in (None, 1.0, 2.0, 3.0, 8.0, 12.0, 16.0):
                        try:
                            want = S.plan(npts, rate, per_lap, wlen, mult)
                        except ValueError:
                            with pytest.raises(ValueError):
                                VS.plan(npts, rate, per_lap, wlen, mult)
                            continue
                        assert VS.plan(npts, rate, per_lap, wlen, mult) == want
                        n += 1
    assert n > 3000
    assert VS.plan(3001, 100.0) == (128, 1024, 115, 13, 222)
    assert VS.plan(141, 100.0) == (128, 1024, 115, 13, 2)
    assert VS.plan(6000, 100.0, wlen=1.92)[0] == 128 and VS.plan(6000, 100.0, mult=3.0)[1] == 256 and VS.plan(6000, 100.0, mult=12.0)[1] == 1024
    for bad in ((127, 100.0, 0.9), (140, 100.0, 0.9), (3001, 100.0, 1.0), (3001, 100.0, 1.5), (3001, 100.0, -0.1)):
        with pytest.raises(ValueError):
            VS.plan(*bad)
    f, t = VS.axes(3001, 100.0, 128, 1024, 13)
    wf, wt = S.axes(3001, 100.0, 128, 1024, 13)
    assert np.array_equal(f, wf) and np.array_equal(t, wt) and f[-1] == 50.0 and len(f) == 512 and len(t) == 222
    assert VS.TILE_FRAMES == 32 and VS.tile_frames(128) == 32 and VS.tile_frames(256) == 16 and VS.tile_frames(512) == 8
    header = (ROOT / "include" / "volpick_hip.h").read_text()
    assert int(re.search(r"#define VP_SPECTROGRAM_TILE_FRAMES (\d+)", header).group(1)) == VS.TILE_FRAMES


@pytest.mark.parametrize("dbscale", (False, True))
def test_the_bound_has_teeth_float32_windowing_and_transform_exceed_it(dbscale):
    x = S.signal(3001, 22, 100.0)
    want, _, _, A = S.spectrogram_f64(x, 100.0, dbscale=dbscale)
    # what the kernel is allowed: the float64 answer rounded once to float32
    assert S.ratio(want.astype(np.float32), want, A, dbscale) <= 0.5 + 1e-9
    single, _, _, _ = S.spectrogram_f64(x, 100.0, dbscale=dbscale, _dtype=np.float32)
    r = S.ratio(single.astype(np.float32), want, A, dbscale)
    print(f"dbscale {dbscale}: float32 windowing and transform: worst |got - want| / bound = {r:.3e}")
    assert r > 10.0
    # a float32 mean of counts around 1e6 exceeds it as well
    c = np.round(S.signal(3001, 23, 100.0, offset=1e6)).astype(np.int32)
    want, _, _, A = S.spectrogram_f64(c, 100.0, dbscale=dbscale)
    shifted, _, _, _ = S.spectrogram_f64(c, 100.0, dbscale=dbscale, _mean=np.float64(c.astype(np.float32).mean(dtype=np.float32)))
    r = S.ratio(shifted.astype(np.float32), want, A, dbscale)
    print(f"dbscale {dbscale}: float32 mean of counts around 1e6: worst |got - want| / bound = {r:.3e}")
    assert r > 10.0
    # exact values: a NaN that is not one, a zero column that is not zero
    bad = want.astype(np.float32).copy()
    bad[3, 5] = np.nan
    assert S.ratio(bad, want, A, dbscale) == math.inf


def test_restatement_edges_nan_inf_zeros_and_frame_ranges():
    x = S.signal(3001, 24, 100.0)
    full, f, t, A = S.spectrogram_f64(x, 100.0)
    part, f2, t2, A2 = S.spectrogram_f64(x, 100.0, frames=(31, 66))
    assert np.array_equal(part, full[:, 31:66]) and np.array_equal(t2, t[31:66]) and np.array_equal(A2, A[31:66])
    for v in (np.nan, np.inf):
        y = x.copy()
        y[1500] = v
        assert np.isnan(S.spectrogram_f64(y, 100.0)[0]).all()
    z = np.concatenate([np.round(x[:1200]), np.zeros(400), -np.round(x[:1200])])  # the mean is exactly 0
    amp = S.spectrogram_f64(z, 100.0)[0]
    db = S.spectrogram_f64(z, 100.0, dbscale=True)[0]
    zero = (amp == 0).all(axis=0)
    assert zero.sum() >= 20 and np.isneginf(db[:, zero]).all() and np.isfinite(db[:, ~zero]).all()


# ---------------------------------------------------------------------------------------------- the host checks of the C entry
VP_OK, VP_ERR_INVALID, VP_ERR_UNSUPPORTED = 0, -1, -4
GOOD = dict(in_null=0, out_null=0, kind=0, n_series=1, stride=3001, n=3001, rate=100.0, nfft=128, pad=1024, hop=13, db=0, first=0,
            count=222)


def host_cases():
    """(label, arguments, expected code)"""
    def c(label, code, **kw):
        return label, {**GOOD, **kw}, code

    out = [c("good", VP_OK), c("every frame of a (3, N) block", VP_OK, n_series=3, stride=4000),
           c("the last frame alone", VP_OK, first=221, count=1), c("an empty range at the end", VP_OK, first=222, count=0),
           c("null input", VP_ERR_INVALID, in_null=1), c("null output", VP_ERR_INVALID, out_null=1),
           c("kind -1", VP_ERR_INVALID, kind=-1), c("kind 3", VP_ERR_INVALID, kind=3),
           c("no series", VP_ERR_INVALID, n_series=0),
           c("n < nfft", VP_ERR_INVALID, n=127, stride=127, count=0),
           c("hop 0", VP_ERR_INVALID, hop=0), c("hop > nfft", VP_ERR_INVALID, hop=129), c("hop -3", VP_ERR_INVALID, hop=-3),
           c("nfft 100", VP_ERR_INVALID, nfft=100), c("pad 1000", VP_ERR_INVALID, pad=1000), c("pad < nfft", VP_ERR_INVALID, pad=64),
           c("nfft 0", VP_ERR_INVALID, nfft=0), c("pad 0", VP_ERR_INVALID, pad=0),
           c("223 frames", VP_ERR_INVALID, count=223), c("first -1", VP_ERR_INVALID, first=-1, count=1),
           c("range past the end", VP_ERR_INVALID, first=200, count=23), c("count -1", VP_ERR_INVALID, count=-1),
           c("first far past the end", VP_ERR_INVALID, first=2**62, count=2**62),
           c("stride < n", VP_ERR_INVALID, stride=3000), c("rate 0", VP_ERR_INVALID, rate=0.0),
           c("rate -100", VP_ERR_INVALID, rate=-100.0), c("rate nan", VP_ERR_INVALID, rate=math.nan),
           c("rate inf", VP_ERR_INVALID, rate=math.inf), c("dbscale 2", VP_ERR_INVALID, db=2),
           c("nfft 16", VP_ERR_UNSUPPORTED, nfft=16, pad=128, hop=2, count=10),
           c("nfft 1024", VP_ERR_UNSUPPORTED, nfft=1024, pad=1024, hop=100, count=10),
           c("pad / nfft 32", VP_ERR_UNSUPPORTED, nfft=32, pad=1024, hop=4, count=10),
           c("pad 8192", VP_ERR_UNSUPPORTED, nfft=512, pad=8192, hop=52, count=10),
           c("65536 series", VP_ERR_UNSUPPORTED, n_series=65536)]
    for nfft in (32, 64, 128, 256, 512):  # every supported window, ratio and the extreme hops: the LDS layout must fit
        for ratio in (1, 2, 4, 8, 16):
            if nfft * ratio > 4096:
                continue
            for hop in (1, nfft // 10 + 1, nfft):
                n = nfft + 70 * hop
                out.append(c(f"nfft {nfft} pad {nfft * ratio} hop {hop}", VP_OK, nfft=nfft, pad=nfft * ratio, hop=hop, n=n, stride=n,
                             count=71))
    return out


def test_host_checks_of_vp_spectrogram_under_the_sanitizers(tmp_path):
    cases = host_cases()
    keys = ("in_null", "out_null", "kind", "n_series", "stride", "n", "rate", "nfft", "pad", "hop", "db", "first", "count")
    (tmp_path / "cases.txt").write_text("".join(
        " ".join(float(a[k]).hex() if k == "rate" else str(a[k]) for k in keys) + "\n" for _, a, _ in cases))
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/llvm/bin/clang++")
    exe = tmp_path / "spectrogram_host_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-I", str(ROOT / "volpick_amd" / "csrc"),
           str(ROOT / "tests" / "spectrogram_host_check.cpp"), "-o", str(exe)]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + sanitize, capture_output=True).returncode != 0:  # no sanitizer runtime for this compiler
        print("sanitizer build failed; building without")
        subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"{len(cases)} cases" and len(lines) == len(cases) + 1
    for (label, a, want), line in zip(cases, lines):
        rc, named, jp, total, lds, xs_cap, nres, scale = line.split()
        assert int(rc) == want, (label, line)
        if want != VP_OK:
            assert named == "1", (label, line)
            continue
        nfft, pad, hop = a["nfft"], a["pad"], a["hop"]
        tile = min(32, 4096 // nfft)
        assert int(jp) == tile and int(total) == (a["n"] - (nfft - hop)) // hop and int(nres) == pad // nfft // 2 + 1, (label, line)
        cap = (tile - 1) * hop + nfft
        assert int(xs_cap) == cap + cap % 2, (label, line)
        assert int(lds) == 8 * int(xs_cap) + 16 * (int(nres) * nfft + nfft // 2) + 16 * tile * (nfft + 1) <= 160 * 1024, (label, line)
        w = np.hanning(nfft)
        assert abs(float.fromhex(scale) * a["rate"] * (w**2).sum() - 1.0) < 1e-14, (label, line)
