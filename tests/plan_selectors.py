"""The documented plan selectors (include/volpick_hip.h: vp_config.plan_flags) that must build and stay oracle-grade:
tests/test_gpu_parity_wide.py runs each, tools/plan_table.py and tests/test_gpu_eqt_plan_table.py record EQTransformer's plans."""
PLAN_SELECTORS = {
    "phasenet": [(1,), (0, 1), (0, 0, 0, 1), (0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 2),
                 (0, 0, 0, 0, 0, 3), (0, 0, 0, 0, 0, 8), (0, 0, 0, 0, 0, 0, 1), (0, 4)],
    "eqtransformer": [(1,), (0, 0, 1), (0, 0, 2), (0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0, 2)] +
                     [(0, 0, 0, 0, 0, 0, 0, 1 << b) for b in range(12)] + [(0, 0, 0, 0, 0, 0, 0, 0x1F0), (0, 0, 0, 0, 0, 0, 0, 0xF)] +
                     [(0, 4), (0, 4, 0, 0, 0, 0, 0, 1024)],
}
