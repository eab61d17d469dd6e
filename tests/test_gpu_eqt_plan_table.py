"""What EQTransformer's host planner builds, per plan selector: step names in order, the algorithmic flops and the issued
work of every step (whole row and two kept ranges), and the debug-tensor table -- the parts of a plan that no numerical
test sees (step order, bench.py's roofline inputs, which tensors a plan keeps).  tests/golden/eqt_plan_table.json was
written by tools/plan_table.py with the library as it stood before the planners moved onto the shared fuse-site helpers;
the library must still give exactly that.  Doubles compare with ==: they are sums of the same literals in the same order.
Handles are created and released, nothing is launched."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

_spec = importlib.util.spec_from_file_location("plan_table", ROOT / "tools" / "plan_table.py")
plan_table = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_table)

GOLDEN = json.loads((ROOT / "tests" / "golden" / "eqt_plan_table.json").read_text())
SELECTORS = plan_table.selectors()


def test_the_golden_table_covers_every_selector():
    assert sorted(GOLDEN) == sorted(plan_table.key(f) for f in SELECTORS)


@pytest.mark.parametrize("flags", SELECTORS, ids=[plan_table.key(f) for f in SELECTORS])
def test_plan_is_the_recorded_one(flags):
    want, got = GOLDEN[plan_table.key(flags)], plan_table.plan_of(flags)
    assert [s["name"] for s in got["steps"]] == [s["name"] for s in want["steps"]]
    for g, w in zip(got["steps"], want["steps"]):
        assert g == w, g["name"]  # (no "issued_work_for_range": every range gives the step's "issued_work")
    assert got["tensors"] == want["tensors"]
