"""The released weights are the only hot-path DATA the reference pins (the reference's
Final_models/**/volpick*.{pt,json}.v1).  tests/golden/weights.sha256 holds one SHA-256 per tensor and per metadata JSON,
computed from the reference's own files, in their state-dict order, by tools/convert_weights.py; here they are recomputed
from what the package ships.  The reference never ships, the digests do."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("convert_weights", ROOT / "tools" / "convert_weights.py")
cw = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cw)

SETS = [(model, name, sub) for model, entries in cw.SETS.items() for sub, name in entries]


def _golden():
    out = {}  # insertion order = the order of the reference's state dicts
    for ln in (ROOT / "tests" / "golden" / "weights.sha256").read_text().splitlines():
        if ln and not ln.startswith("#"):
            digest, key = ln.split("  ", 1)
            out[key] = digest
    return out


def _shipped(model, name):
    d = ROOT / "volpick_amd" / "weights" / model
    with np.load(d / f"{name}.npz") as z:
        arrays = {k: z[k] for k in z.files}
    return arrays, json.loads((d / f"{name}.json").read_text())


def test_digest_file_covers_exactly_the_four_released_sets():
    keys = _golden()
    assert len(keys) == 2 * (111 + 1) + 2 * (249 + 1)  # Appendix B: 111 / 249 state-dict entries + one JSON each
    assert {k.split("/")[0] for k in keys} == {"phasenet", "eqtransformer"}
    assert len(set(keys.values())) > 600  # distinct tensors have distinct digests (a few BN counters coincide)


@pytest.mark.parametrize("model,name,sub", SETS)
def test_shipped_weights_match_the_reference_digests(model, name, sub):
    golden = _golden()
    arrays, meta = _shipped(model, name)
    want = {k: v for k, v in golden.items() if k.startswith(f"{model}/{name}.")}
    got = dict(ln.split("  ", 1)[::-1] for ln in cw.digest_lines(model, name, arrays, meta))
    assert got.keys() == want.keys(), "tensor names / count differ from the released state dict"
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)} tensors differ from the reference's release, e.g. {bad[:3]}"
    n_floats = sum(a.size for a in arrays.values() if a.dtype == np.float32)
    assert n_floats == (269_675 if model == "phasenet" else 378_823)


def test_a_flipped_bit_is_caught():
    arrays, meta = _shipped("phasenet", "volpick")
    a = arrays["inc.weight"].copy()
    a.view(np.uint32).flat[0] ^= 1
    assert cw.tensor_digest("inc.weight", a) != cw.tensor_digest("inc.weight", arrays["inc.weight"])
    assert cw.json_digest(dict(meta, version="2")) != cw.json_digest(meta)


@pytest.mark.parametrize("model,name,sub", SETS)
def test_shipped_weights_are_the_reference_files_in_order(model, name, sub):
    """Every tensor of the shipped set, in the order of the reference's state dict, with its name, dtype, shape and bytes,
    and the metadata JSON, against the digests taken from the reference's .pt.v1 / .json.v1 files."""
    want = [(k, v) for k, v in _golden().items() if k.startswith(f"{model}/{name}.")]
    arrays, meta = _shipped(model, name)
    got = [ln.split("  ", 1)[::-1] for ln in cw.digest_lines(model, name, arrays, meta)]
    assert [tuple(x) for x in got] == want
