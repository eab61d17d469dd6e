"""Teeth of the float64 checks of preprocessing and stacking (tests/prepost_f64.py), on CPU.  This runs no kernel: it covers the
bounds the GPU test (tests/test_gpu_prepost_f64.py) holds the kernels to.

* Plain fp32 (torch ``batch_pre``, numpy ``reassemble``) stays within the bounds on every configuration, input and case.
* An fp32 emulation with ONE fault at a time leaves them: preprocessing by at least ``TEETH`` x the bound on some input of every
  configuration the fault applies to; stacking by a broken NaN pattern or bound on some case of the table.  ``TEETH`` is a
  condition on the sharpness of the bound, not a measurement: a fault that falls below it needs an input that shows it."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import constants as OC
from oracle import pipeline as OP
from tests.prepost_f64 import (CONFIGS, IN_SAMPLES, STACK_CASES, effective, pre64, pre_inputs, pre_ratio, stack64, stack_case_id,
                               stack_ratio, valid_range)

TEETH = 4.0
F32 = np.float32


def pre32(x, model_name, norm, per_comp, fault=None):
    """annotate_batch_pre in fp32 numpy (pairwise sums: fp32-accurate, not the kernel's order), with one named fault."""
    T = x.shape[2]
    norm, per = effective(model_name, norm, per_comp)
    if fault == "amp_scope_swapped":
        per = not per
    if fault == "mean_padded_length":
        mean = x.sum(-1, keepdims=True, dtype=F32) / F32(1024 * math.ceil(T / 1024))
    elif fault == "mean_misses_last":
        mean = x[..., :-1].sum(-1, keepdims=True, dtype=F32) / F32(T)
    else:
        mean = x.sum(-1, keepdims=True, dtype=F32) / F32(T)
    d = (x - mean).astype(F32)
    ax = -1 if per else (-2, -1)
    if norm == "peak":
        a = x if fault == "peak_of_raw" else d
        amp = a.max(ax, keepdims=True) if fault == "peak_positive_side" else np.abs(a).max(ax, keepdims=True)
    else:
        n = T if per else 3 * T
        amp = np.sqrt((d * d).sum(ax, keepdims=True, dtype=F32) / F32(n if fault == "std_T_for_T-1" else n - 1))
    den = amp if fault == "no_eps" else (amp + F32(OC.NORM_EPS)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o = (d / den).astype(F32)
        if model_name == "EQTransformer":
            n = OC.EQT_TAPER_SAMPLES
            ang = np.linspace(np.pi, 2 * np.pi, n, endpoint=fault != "taper_without_endpoint").astype(F32)
            tap = (F32(0.5) * (F32(1) + np.cos(ang))).astype(F32)
            sh = 1 if fault == "taper_shifted" else 0
            o[..., sh:n + sh] *= tap
            o[..., T - n - sh:T - sh] *= tap if fault == "taper_right_not_flipped" else tap[::-1]
    return o


PRE_FAULTS = {  # fault -> does it apply to (model name, effective norm)?
    "mean_padded_length": lambda m, n: True,
    "mean_misses_last": lambda m, n: True,
    "std_T_for_T-1": lambda m, n: n == "std",
    "peak_of_raw": lambda m, n: n == "peak",
    "peak_positive_side": lambda m, n: n == "peak",
    "amp_scope_swapped": lambda m, n: True,
    "no_eps": lambda m, n: True,
    "taper_without_endpoint": lambda m, n: m == "EQTransformer",
    "taper_shifted": lambda m, n: m == "EQTransformer",
    "taper_right_not_flipped": lambda m, n: m == "EQTransformer",
}


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fp32_preprocessing_is_within_the_bound_and_every_fault_is_not(cfg):
    cid, name, norm, per_comp = cfg
    T = IN_SAMPLES[name]
    eff_norm = effective(name, norm, per_comp)[0]
    inputs = pre_inputs(T, seed=11, peak_only=eff_norm == "peak")
    stub = SimpleNamespace(name=name, norm=norm, norm_amp_per_comp=per_comp)
    worst = {f: 0.0 for f, applies in PRE_FAULTS.items() if applies(name, eff_norm)}
    for iname, x in inputs.items():
        want, bound = pre64(x, name, norm, per_comp)
        assert np.isfinite(want).all() and np.isfinite(bound).all()
        r_torch = pre_ratio(OP.batch_pre(stub, torch.from_numpy(x)).numpy(), want, bound)
        r_np = pre_ratio(pre32(x, name, norm, per_comp), want, bound)
        print(f"{cid:12s} {iname:11s} torch-fp32 {r_torch:8.3f}  numpy-fp32 {r_np:8.3f}  of the bound")
        assert r_torch <= 1.0 and r_np <= 1.0, (cid, iname, r_torch, r_np)
        for f in worst:
            worst[f] = max(worst[f], pre_ratio(pre32(x, name, norm, per_comp, fault=f), want, bound))
    for f, r in worst.items():
        print(f"{cid:12s} fault {f:24s} {r:12.4g} x the bound")
    weak = {f: r for f, r in worst.items() if not r >= TEETH}
    assert not weak, f"{cid}: faults the bound does not see by {TEETH} x on any input (add an input that shows them): {weak}"


# ------------------------------------------------------------------------------------------------------------ stacking
def stack32(preds, N, T, overlap, blind_l, blind_r, mode, fault=None):
    """fp32 emulation of stack_kernel's gather (lo, hi, serial sum in window order, tail) with one named fault.  ``preds`` holds
    one spare row behind the last window: what a fault that reads one window too far finds there."""
    step = T - overlap
    n_reg = 0 if N < T else (N - T) // step + 1
    has_tail = int(N >= T and (n_reg - 1) * step + T < N)
    if fault == "blinding_swapped":
        blind_l, blind_r = blind_r, blind_l
    t = np.arange(N)
    hi = np.where(t - blind_l >= 0, (t - blind_l) // step, -1)
    lo_num = t - T + blind_r
    lo = np.where(lo_num < 0, 0, lo_num // step + (0 if fault == "lo_without_plus_1" else 1))
    hi = np.minimum(hi, n_reg if fault == "hi_clamped_to_n_regular" else n_reg - 1)
    n_out = preds.shape[1]
    flat = np.concatenate([preds.ravel(), np.zeros(n_out * T, F32)])  # the kernel indexes flat memory: an offset of T is the next row

    def read(i, off):
        return np.stack([flat[(i * n_out + c) * T + off] for c in range(n_out)])

    acc = np.full((n_out, N), 0.0 if mode == "avg" else -np.inf, F32)
    cnt = np.zeros((n_out, N), np.int64)

    def add(sel, v):
        ok = ~np.isnan(v)
        a = acc[:, sel]
        with np.errstate(invalid="ignore"):
            acc[:, sel] = np.where(ok, (a + v).astype(F32) if mode == "avg" else np.maximum(a, v), a)
        cnt[:, sel] += 1 if fault == "count_before_nan_skip" else ok

    for i in range(int(hi.max()) + 1 if N else 0):
        sel = np.flatnonzero((lo <= i) & (i <= hi))
        if sel.size:
            add(sel, read(i, sel - i * step))
    if has_tail or fault == "tail_without_has_tail":
        j = t - (N - T)
        keep = (j >= blind_l) & ((j <= T - blind_r) if fault == "tail_range_le" else (j < T - blind_r)) & (j >= 0) & (j < T)
        sel = np.flatnonzero(keep)
        if sel.size:
            add(sel, read(n_reg, j[sel]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, (acc / cnt.astype(F32)).astype(F32) if mode == "avg" else acc, np.nan)


STACK_FAULTS = ["hi_clamped_to_n_regular", "lo_without_plus_1", "tail_range_le", "blinding_swapped", "count_before_nan_skip",
                "tail_without_has_tail"]


def _random_preds(n, T, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (n + 1, 2, T)).astype(F32)  # + the spare row of stack32
    if n > 2:
        p[1] = np.nan
        p[n // 2] = np.nan
    return p


def test_fp32_stacking_is_within_the_bound_and_every_fault_is_not():
    T = OC.PN_IN_SAMPLES
    caught = {f: [] for f in STACK_FAULTS}
    for ci, case in enumerate(STACK_CASES(T)):
        N, overlap, bl, br, mode = case
        starts = OP.window_starts(N, T, overlap)
        preds = _random_preds(len(starts), T, seed=100 + ci)
        want, cnt, bound = stack64(preds[:len(starts)], starts, T, N, bl, br, mode)
        nw, fv, lv = valid_range(starts, T, bl, br)
        if nw == 0:
            assert np.isnan(want).all() and (fv, lv) == (-1, -1)
        else:
            assert np.isnan(want[:, :fv]).all() and np.isnan(want[:, lv + 1:]).all()
            # second opinion: the reference pipeline's own fp32 NaN-buffer stacking
            blinded = preds[:nw].transpose(0, 2, 1).copy()
            blinded[:, :bl] = np.nan
            if br:
                blinded[:, T - br:] = np.nan
            ref = OP.reassemble(blinded, starts, T, overlap, mode).T
            full = np.full(want.shape, np.nan, F32)
            full[:, :ref.shape[1]] = ref
            same, r = stack_ratio(full, want, bound)
            print(f"{stack_case_id(case):34s} reassemble: pattern {'ok' if same else 'BROKEN'}, {r:.3f} of the bound, "
                  f"count up to {int(cnt.max())}")
            assert same and r <= 1.0, (case, same, r)
        same, r = stack_ratio(stack32(preds, N, T, overlap, bl, br, mode), want, bound)
        assert same and r <= 1.0, ("emulation without a fault", case, same, r)
        for f in STACK_FAULTS:
            same, r = stack_ratio(stack32(preds, N, T, overlap, bl, br, mode, fault=f), want, bound)
            if not same or r > 1.0:
                caught[f].append(stack_case_id(case))
    for f, cs in caught.items():
        print(f"fault {f:26s} caught by {len(cs):2d} cases: {cs}")
    assert all(caught.values()), {f: len(cs) for f, cs in caught.items()}


def test_stack_cases_serve_both_models():
    """The table keeps its structure at both window lengths: the no-tail case has no tail, its neighbours do, the step-1
    blinding keeps one sample, blinding and N both go down and up along the table."""
    for T in (OC.PN_IN_SAMPLES, OC.EQT_IN_SAMPLES):
        cases = STACK_CASES(T)
        for N, overlap, bl, br, mode in cases:
            assert 0 <= overlap < T and bl >= 0 and br >= 0 and bl + br < T and mode in ("avg", "max")
        tails = [len(OP.window_starts(c[0], T, c[1])) - (0 if c[0] < T else (c[0] - T) // (T - c[1]) + 1) for c in cases]
        assert tails[0] == 0 and tails[2] == 1 and tails[3:6] == [0, 1, 1]
        assert any(c[0] < T for c in cases) and any(T - c[1] == 1 and c[2] + c[3] == T - 1 for c in cases)
        assert any(T - c[1] == 11 for c in cases) and any(c[2] + c[3] > c[1] > 0 for c in cases)
        dn = np.sign(np.diff([c[0] for c in cases]))
        db = np.sign(np.diff([c[2] + c[3] for c in cases]))
        assert (dn > 0).any() and (dn < 0).any() and (db > 0).any() and (db < 0).any()
