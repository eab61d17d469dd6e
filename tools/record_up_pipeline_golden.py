#!/usr/bin/env python3
"""Record tests/golden/phasenet_up_pipeline.npz: what the PhaseNet window kernel of the library IN PLACE computes, bit for bit.

The fixture pins the output of a build across a change that must not alter a single bit (a reordering of the level-0 up
path's schedule, say): check out the commit whose results are the reference, build it, run this script on the GPU, commit the
file, then change the kernel.  tests/test_gpu_phasenet_up_pipeline.py compares with np.array_equal.

    python tools/record_up_pipeline_golden.py [OUT.npz]        (default: tests/golden/phasenet_up_pipeline.npz)

Only outputs are stored; the inputs are the seeded synthetic windows / stream of `cases()` below, which the test regenerates.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows  # noqa: E402

T = 3001
BATCHES = {1: 5101, 3: 5103, 17: 5117}          # batch size -> seed of its windows
STREAM_N, STREAM_SEED, STREAM_OVERLAP = 5400, 5201, 1500  # windows at 0, 1501 and 2399 (the tail, flush with the end: 3002 > N - T)


def windows(B):
    return synthetic_windows(B, T, seed=BATCHES[B])


def stream():
    return synthetic_stream_array(STREAM_N, seed=STREAM_SEED, n_events=2)[0]


def stream_outputs(model):
    """Stacked rows (vp_annotate) and trigger columns (the submit / collect path) of the device-resident stream."""
    import torch

    data = torch.from_numpy(stream()).cuda()
    args = model._argdict(dict(overlap=STREAM_OVERLAP, blinding=(0, 0), stacking="avg"))
    rows, fv, lv, nw = model._annotate_block(data, args)
    specs = model._trigger_specs(args)
    job = model._submit_block(0, data, args, specs, 8192)
    (spec_of, on, off, peak, val), nw2 = model._collect_block(job, args, specs, columns=True)
    return dict(stream_rows=rows.cpu().numpy(), stream_meta=np.array([fv, lv, nw, nw2], np.int64), pick_spec=spec_of,
                pick_on=on, pick_off=off, pick_peak=peak, pick_value=val)


def main():
    from volpick_amd import PhaseNet

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "phasenet_up_pipeline.npz"
    model = PhaseNet.from_pretrained("volpick").cuda()
    arrays = {f"y{B}": np.asarray(model._forward_raw(windows(B), preprocess=True)) for B in BATCHES}
    arrays.update(stream_outputs(model))
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(out, {k: v.shape for k, v in arrays.items()}, "windows of the stream:", arrays["stream_meta"][2],
          "picks:", len(arrays["pick_on"]), "bytes:", out.stat().st_size)


if __name__ == "__main__":
    main()
