"""The level-0 up path of pn_window_kernel runs a tile's epilogue (1 x 1 conv, softmax, stores to y) one phase late, under
the next tile's fragment reads, with one drain epilogue behind the loop.  Only the schedule moved: y must be what the build
before that change computed, BIT FOR BIT.  tests/golden/phasenet_up_pipeline.npz holds that build's outputs; it was recorded
on the GPU from the parent commit's library with tools/record_up_pipeline_golden.py (inputs are seeded, only outputs are
stored -- the seeds below are the script's).

What a wrong deferral looks like: the last tile (samples from about 2800 on) never stored or stored twice with another
tile's sums (the drain), the first tile's samples wrong (the phase that has no epilogue owed yet), a sample left unwritten
(it keeps what the previous forward pass left in the output buffer), a poisoned window's NaN lost on the way to the late
epilogue."""
from pathlib import Path

import numpy as np
import pytest
import torch

from volpick_amd import PhaseNet
from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows

pytestmark = pytest.mark.gpu

T = 3001
SEEDS = {1: 5101, 3: 5103, 17: 5117}
STREAM_N, STREAM_SEED, STREAM_OVERLAP = 5400, 5201, 1500
LAST_TILE = 2800  # the twelfth tile of 256 samples starts at 2808: its epilogue is the one behind the loop


@pytest.fixture(scope="module")
def golden():
    with np.load(Path(__file__).parent / "golden" / "phasenet_up_pipeline.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def model():
    return PhaseNet.from_pretrained("volpick").cuda()


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got[..., :8], want[..., :8]), f"{what}: first tile"
    assert np.array_equal(got[..., LAST_TILE:], want[..., LAST_TILE:]), f"{what}: last tile (the drain epilogue)"
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("B", [1, 3, 17])
def test_y_is_bit_identical_to_the_parent_build(model, golden, B):
    x = synthetic_windows(B, T, seed=SEEDS[B])
    # another input through the same model object first: a sample the kernel then leaves unwritten keeps that run's value
    other = np.asarray(model._forward_raw(synthetic_windows(B, T, seed=SEEDS[B] + 1000), preprocess=True))
    assert not np.array_equal(other, golden[f"y{B}"])
    assert_same(np.asarray(model._forward_raw(x, preprocess=True)), golden[f"y{B}"], f"B={B}, host windows")
    # ... and with the windows and y resident on the device (the kernel writes the caller's buffer directly)
    xd = torch.from_numpy(x).cuda()
    del other
    other = model._forward_raw(torch.from_numpy(synthetic_windows(B, T, seed=SEEDS[B] + 2000)).cuda(), preprocess=True)
    del other  # (the caching allocator hands the same block to the next y)
    assert_same(model._forward_raw(xd, preprocess=True).cpu().numpy(), golden[f"y{B}"], f"B={B}, device windows")


def test_a_nonfinite_window_stays_nan_and_does_not_leak(model, golden):
    x = synthetic_windows(3, T, seed=SEEDS[3])
    x[1, 2, 1234] = np.nan
    model._forward_raw(synthetic_windows(3, T, seed=SEEDS[3] + 1000), preprocess=True)  # finite values in the output buffer
    got = np.asarray(model._forward_raw(x, preprocess=True))
    assert np.isnan(got[1]).all()  # every sample of every row, the last tile's (drain) included
    for w in (0, 2):
        assert_same(got[w], golden["y3"][w], f"window {w} beside the poisoned one")


def test_stream_rows_and_picks_are_bit_identical_to_the_parent_build(model, golden):
    """Three windows cut from a device-resident stream inside the kernel: starts 0, 1501 and 2399 -- the tail window, whose
    grid start 3002 lies beyond N - T, is flush with the end."""
    data = torch.from_numpy(synthetic_stream_array(STREAM_N, seed=STREAM_SEED, n_events=2)[0]).cuda()
    args = model._argdict(dict(overlap=STREAM_OVERLAP, blinding=(0, 0), stacking="avg"))
    assert 2 * (T - STREAM_OVERLAP) > STREAM_N - T
    rows, fv, lv, nw = model._annotate_block(data, args)
    assert [fv, lv, nw] == golden["stream_meta"][:3].tolist() and nw == 3
    assert np.array_equal(rows.cpu().numpy(), golden["stream_rows"], equal_nan=True)
    specs = model._trigger_specs(args)
    (spec_of, on, off, peak, val), nw2 = model._collect_block(model._submit_block(0, data, args, specs, 8192), args, specs, columns=True)
    assert nw2 == golden["stream_meta"][3] == 3
    assert len(on) == len(golden["pick_on"]) > 0
    for got, key in ((spec_of, "pick_spec"), (on, "pick_on"), (off, "pick_off"), (peak, "pick_peak"), (val, "pick_value")):
        assert np.array_equal(got, golden[key]), key
