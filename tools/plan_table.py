#!/usr/bin/env python3
"""What EQTransformer's host planner builds for every plan selector, without launching anything: the step names in order,
each step's algorithmic flops and issued work (whole row and two kept ranges), and the debug-tensor table.  These are the
parts of a plan that no numerical test sees: step order, bench.py's roofline inputs, which tensors a plan keeps.  A step
carries "issued_work_for_range" only where a range's answer differs from its "issued_work" (the time-tiled decoder tail).

usage: plan_table.py OUT.json      (the library under VOLPICK_HIP_LIB, or the tree's own)
tests/test_gpu_eqt_plan_table.py compares plan_table() with tests/golden/eqt_plan_table.json."""
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import volpick_amd as va  # noqa: E402
from tests.plan_selectors import PLAN_SELECTORS  # noqa: E402
from volpick_amd import _lib  # noqa: E402

RANGES = [(0, 0), (500, 5500), (250, 5750)]


def selectors():
    return [()] + list(PLAN_SELECTORS["eqtransformer"])


def key(flags):
    return ".".join(map(str, flags)) or "default"


def _work(call, *args):
    w = _lib.VpIssuedWork()
    _lib.check(call(*args, C.byref(w)))
    return [w.mfma_f32_flop, w.mfma_bf16_flop, w.valu_flop]


def plan_of(flags):
    """The plan of one selector, created as tests/test_gpu_parity_wide.py creates it; nothing is launched."""
    lib = _lib.load()
    m = va.EQTransformer.from_pretrained("volpick")
    m._plan_flags = flags
    m.cuda()
    try:
        h, steps, tensors = m._handle, [], []
        for i in range(lib.vp_step_count(h)):
            name, fl = C.c_char_p(), C.c_double()
            _lib.check(lib.vp_step_info(h, i, C.byref(name), C.byref(fl)))
            step = {"name": name.value.decode(), "flops_per_window": fl.value, "issued_work": _work(lib.vp_step_issued_work, h, i)}
            ranges = {f"{lo},{hi}": _work(lib.vp_step_issued_work_for_range, h, i, lo, hi) for lo, hi in RANGES}
            if any(w != step["issued_work"] for w in ranges.values()):
                step["issued_work_for_range"] = ranges
            steps.append(step)
        for i in range(lib.vp_debug_tensor_count(h)):
            name, c, l = C.c_char_p(), C.c_int(), C.c_int()
            _lib.check(lib.vp_debug_tensor_info(h, i, C.byref(name), C.byref(c), C.byref(l)))
            tensors.append([name.value.decode(), c.value, l.value])
        return {"steps": steps, "tensors": tensors}
    finally:
        m._release()


def plan_table():
    return {key(f): plan_of(f) for f in selectors()}


def dumps(table):
    """One line per selector; repr of a double round-trips exactly."""
    return "{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in table.items()) + "\n}\n"


if __name__ == "__main__":
    Path(sys.argv[1]).write_text(dumps(plan_table()))
