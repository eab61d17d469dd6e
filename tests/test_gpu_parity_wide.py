"""GPU parity, widened: both released weight sets of both models, a regression bar beside the
north-star bar, and inputs / weights far from the O(1) activations of volpick_amd.synthetic through the DEFAULT plans
(the bf16-piece kernels) against the CPU oracle.

Two bars.  CONTRACT = 1e-4 absolute on probabilities (BASELINE.json north_star).  REGRESSION = 3e-5: the measured
distance to the oracle is 1.1e-5 at most (profiles/archive/r02_err_check_vs_oracle.txt), so a change that quintuples it -- one
dropped piece product, one wrong rounding mode -- fails here long before it reaches the contract bar."""
import copy

import numpy as np
import pytest
import torch

import volpick_amd as va
from oracle import pipeline as OP
from oracle.models import load_pretrained
from tests.plan_selectors import PLAN_SELECTORS
from volpick_amd.synthetic import synthetic_stream_array, synthetic_windows

pytestmark = pytest.mark.gpu
CONTRACT = 1e-4
REGRESSION = 3e-5

MODELS = {"phasenet": va.PhaseNet, "eqtransformer": va.EQTransformer}
PAIRS = [(m, w) for m in MODELS for w in ("volpick", "volpick_95train")]


def _as_array(y):
    """model(x) -> (B, 3, T) ndarray (EQTransformer returns a tuple of three (B, T) tensors)."""
    if isinstance(y, tuple):
        return np.stack([t.detach().cpu().numpy() for t in y], 1)
    return y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)


def _check(got, want, what, bar=REGRESSION):
    err = float(np.abs(got - want).max())
    print(f"{what}: max|hip - oracle| = {err:.3e}")
    assert np.isfinite(got).all(), what
    assert err < CONTRACT, f"{what}: {err:.3e} breaks the north-star bar {CONTRACT}"
    assert err < bar, f"{what}: {err:.3e} is inside the contract but beyond the regression bar {bar} (was <= 1.1e-5)"
    return err


@pytest.fixture(scope="module", params=PAIRS, ids=[f"{m}-{w}" for m, w in PAIRS])
def pair(request):
    name, weights = request.param
    model = MODELS[name].from_pretrained(weights).cuda()
    yield name, weights, model, load_pretrained(name, weights)
    model._release()


# ---- (a) both weight sets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 256])
def test_forward_parity_both_weight_sets(pair, B):
    name, weights, model, oracle = pair
    x = synthetic_windows(B, model.in_samples, seed=4100 + B)
    xn = OP.batch_pre(oracle, torch.from_numpy(x))
    with torch.no_grad():
        want = _as_array(oracle(xn))
    _check(_as_array(model(xn.cuda())), want, f"{name}/{weights} forward B={B}")
    # device-side annotate_batch_pre on the raw windows gives the same predictions
    _check(model._forward_raw(x, preprocess=True), want, f"{name}/{weights} forward B={B}, in-kernel preprocessing")


def test_annotate_parity_both_weight_sets(pair):
    name, weights, model, oracle = pair
    T = model.in_samples
    overlap, blinding = (1500, (0, 0)) if name == "phasenet" else (5500, (500, 500))
    n = T + (T - overlap) * 19 + 123  # 20 regular windows + a tail window
    data, _, _ = synthetic_stream_array(n, seed=4200, n_events=5)
    want = OP.annotate_array(oracle, data, overlap=overlap, blinding=blinding, stacking="avg")
    args = model._argdict(dict(overlap=overlap, blinding=blinding, stacking="avg"))
    out, fv, lv, nw = model._annotate_block(data, args)
    out = out.cpu().numpy()
    assert nw == len(OP.window_starts(n, T, overlap)) == 21
    for i, (label, off, tr) in enumerate(want):
        assert off == fv and len(tr) == lv - fv + 1, (label, off, fv, len(tr), lv)
        got = out[i, fv:lv + 1]
        assert np.array_equal(np.isnan(got), np.isnan(tr))
        ok = ~np.isnan(tr)
        _check(got[ok], tr[ok], f"{name}/{weights} annotate {label}")


def test_classify_picks_both_weight_sets(pair):
    name, weights, model, oracle = pair
    T = model.in_samples
    overlap, blinding = (1500, (0, 0)) if name == "phasenet" else (5500, (500, 500))
    n = T + (T - overlap) * 31
    data, _, _ = synthetic_stream_array(n, seed=4300, n_events=6)
    want = sorted(OP.classify_array(oracle, data, overlap=overlap, blinding=blinding)["picks"])
    args = model._argdict(dict(overlap=overlap, blinding=blinding, stacking="avg"))
    specs = [s for s in model._trigger_specs(args) if s[1] != "Detection"]
    got, _ = model._classify_block(data, args, specs)
    got = sorted((specs[si][1], on, off, pk, v) for si, on, off, pk, v in got)
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2], (g, w)  # phase, onset, end: identical samples
        assert g[3] == w[3], (g, w)                                    # peak sample
        assert abs(g[4] - w[4]) < REGRESSION


# ---- (c) adversarial inputs through the default plans -----------------------------------------------------------------
def _adversarial(kind, B, T, seed):
    rng = np.random.default_rng(seed)
    x = synthetic_windows(B, T, seed=seed)
    if kind == "counts_dc_1e6":  # raw digitiser counts on a 1e6 offset (fp32 keeps integers below 2^24 exactly)
        x = np.round(x / np.abs(x).max(axis=(1, 2), keepdims=True) * 40_000.0) + 1.0e6
    elif kind == "clipped_square":  # a saturated sensor: +-A with a few transitions per second
        t = np.arange(T) / 100.0
        f = rng.uniform(0.2, 3.0, size=(B, 3, 1))
        x = np.sign(np.sin(2 * np.pi * f * t[None, None, :] + rng.uniform(0, 6, size=(B, 3, 1)))) * 32767.0
        x[x == 0] = 32767.0
    elif kind == "constant_channel":  # a dead component (integer level: its mean is exact, the demeaned row is 0)
        x[:, 1, :] = 1234.0
    elif kind == "spike_1e9":  # one glitch sample dwarfs everything else
        x = x / np.abs(x).max(axis=(1, 2), keepdims=True)
        for b in range(B):
            x[b, b % 3, int(rng.integers(50, T - 50))] = 1.0e9
    elif kind == "all_zero":
        x[:] = 0.0
        x[0] = synthetic_windows(1, T, seed=seed + 1)[0]  # one ordinary window beside them
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


@pytest.fixture(scope="module", params=list(MODELS))
def default_pair(request):
    model = MODELS[request.param].from_pretrained("volpick").cuda()
    yield request.param, model, load_pretrained(request.param)
    model._release()


@pytest.mark.parametrize("kind", ["counts_dc_1e6", "clipped_square", "constant_channel", "spike_1e9", "all_zero"])
def test_adversarial_inputs_default_plan(default_pair, kind):
    """Raw windows -> in-kernel annotate_batch_pre -> the bf16-piece forward kernels, against the oracle fed the same
    raw windows.  The normalised inputs differ by the rounding of the mean (the reduction orders differ), which the
    1e6-offset and the 1e9-spike cases amplify; the bar for every case is the regression bar."""
    name, model, oracle = default_pair
    x = _adversarial(kind, 6, model.in_samples, seed=4400 + len(kind))
    xn = OP.batch_pre(oracle, torch.from_numpy(x.copy()))
    with torch.no_grad():
        want = _as_array(oracle(xn))
    assert np.isfinite(want).all()
    _check(model._forward_raw(x, preprocess=True), want, f"{name} {kind}")


# ---- (c') activations far from O(1) inside the bf16-piece layers ------------------------------------------------------
# ReLU, MaxPool and the folded BatchNorm are positively homogeneous, so scaling the affine output of one layer by s and
# the weights of the next by 1 / s leaves the network's function unchanged while the activations BETWEEN them sit at s
# times their usual size -- inside layers whose operands are split into three bfloat16 pieces (conv_b3.h b3_split /
# b3_store4: hi = rne(x), mid = rne(x - hi), lo = x - hi - mid).  bfloat16 has fp32's exponent range, so the pieces of
# a value at 1e+-30 are still normal numbers (the lo piece at ~2^-16 of the value); the oracle with the same scaled
# weights is the reference, and the unscaled network's output is the sanity check that the scaling is neutral.
def _scaled_state(model_name, sd, s):
    sd = {k: (v.clone() if torch.is_tensor(v) else np.array(v, copy=True)) for k, v in sd.items()}

    def mul(key, f):
        sd[key] = sd[key] * f

    if model_name == "phasenet":
        # output of down2.down (BatchNorm down_branch.2.3, then ReLU) enters down3.same, the first bf16-piece layer
        mul("down_branch.2.3.weight", s)
        mul("down_branch.2.3.bias", s)
        mul("down_branch.3.0.weight", 1.0 / s)
    else:
        # encoder stage 5 (conv + ReLU + MaxPool) feeds stage 6; decoder stage 4 feeds stage 5 (all three decoders)
        mul("encoder.convs.5.weight", s)
        mul("encoder.convs.5.bias", s)
        mul("encoder.convs.6.weight", 1.0 / s)
        for dec in ("decoder_d", "pick_decoders.0", "pick_decoders.1"):
            mul(f"{dec}.convs.4.weight", s)
            mul(f"{dec}.convs.4.bias", s)
            mul(f"{dec}.convs.5.weight", 1.0 / s)
    return sd


def _scaled_up_path(sd, s):
    """PhaseNet: both inputs of up1.same and of up2.same (the skip rows and the transposed conv's output: the layers that run
    in two K halves over one refilled piece image) at s times their size; every consumer of those tensors divides by s."""
    sd = {k: (v.clone() if torch.is_tensor(v) else np.array(v, copy=True)) for k, v in sd.items()}
    for level, up in ((2, 1), (1, 2)):  # up1.same reads skip 2, up2.same skip 1
        for k in ("weight", "bias"):
            sd[f"down_branch.{level}.1.{k}"] = sd[f"down_branch.{level}.1.{k}"] * s  # BatchNorm of down{level}.same (the skip)
            sd[f"up_branch.{up}.1.{k}"] = sd[f"up_branch.{up}.1.{k}"] * s            # BatchNorm of up{up}.convT
        sd[f"down_branch.{level}.2.weight"] = sd[f"down_branch.{level}.2.weight"] / s  # down{level}.down reads the skip too
        sd[f"up_branch.{up}.2.weight"] = sd[f"up_branch.{up}.2.weight"] / s            # up{up}.same
    return sd


@pytest.mark.parametrize("scale", [1e15, 1e-15])
def test_activations_far_from_unity_in_the_up_path_piece_layers(scale):
    oracle = load_pretrained("phasenet", "volpick")
    m = va.PhaseNet.from_pretrained("volpick")
    big = copy.deepcopy(oracle)
    big.load_state_dict(_scaled_up_path(big.state_dict(), scale), strict=True)
    m.load_state_dict({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _scaled_up_path(m.state_dict(), scale).items()})
    m.cuda()
    try:
        x = synthetic_windows(4, m.in_samples, seed=4600)
        xn = OP.batch_pre(oracle, torch.from_numpy(x))
        with torch.no_grad():
            want = _as_array(big(xn))
            plain = _as_array(oracle(xn))
        assert np.abs(want - plain).max() < 1e-5, "the scaling must be neutral for the oracle itself"
        _check(_as_array(m(xn.cuda())), want, f"phasenet up path x {scale:g}")
    finally:
        m._release()


@pytest.mark.parametrize("scale", [1e20, 1e-20, 1e30, 1e-30])
def test_activations_far_from_unity_in_piece_layers(default_pair, scale):
    name, model, oracle = default_pair
    big = copy.deepcopy(oracle)
    big.load_state_dict(_scaled_state(name, big.state_dict(), scale), strict=True)
    m = MODELS[name].from_pretrained("volpick")
    sd = m.state_dict()
    m.load_state_dict({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _scaled_state(name, sd, scale).items()})
    m.cuda()
    try:
        x = synthetic_windows(4, m.in_samples, seed=4500)
        xn = OP.batch_pre(oracle, torch.from_numpy(x))
        with torch.no_grad():
            want = _as_array(big(xn))
            plain = _as_array(oracle(xn))
        assert np.abs(want - plain).max() < 1e-5, "the scaling must be neutral for the oracle itself"
        _check(_as_array(m(xn.cuda())), want, f"{name} activations x {scale:g}")
    finally:
        m._release()


# ---- (b) the regression bar on the BASELINE batch ---------------------------------------------------------------------
def test_regression_bar_full_batch(default_pair):
    name, model, oracle = default_pair
    x = synthetic_windows(256, model.in_samples, seed=4600)
    xn = OP.batch_pre(oracle, torch.from_numpy(x))
    with torch.no_grad():
        want = _as_array(oracle(xn))
    got = _as_array(model(xn.cuda()))
    err = _check(got, want, f"{name} 256 windows")
    assert float(np.abs(got - want).mean()) < 2e-7, err


# ---- (e) every documented plan selector (include/volpick_hip.h: vp_config.plan_flags) still produces oracle-grade outputs:
# PLAN_SELECTORS (tests/plan_selectors.py) --------


# A/B forms that round 6 removed: the library says so instead of running something else
REMOVED_SELECTORS = {
    "phasenet": [(0, 0, 1), (0, 0, 0, 2), (0, 0, 0, 0, 0, 4), (0, 0, 0, 0, 0, 5), (0, 0, 0, 0, 0, 6), (0, 0, 0, 0, 0, 7), (0, 0, 0, 0, 0, 9)],
    "eqtransformer": [(0, 0, 0, 0, 0, 0, 0, 4096), (0, 0, 3), (0, 0, 0, 1), (0, 0, 0, 0, 0, 0, 0, 8192)],
}
# what the error of a selector removed since then says; every other one says "removed in round 6"
REMOVED_MATCH = {
    ("eqtransformer", (0, 0, 3)): r"plan_flags\[2\] = 3 \(middle kernel with two windows per workgroup in teams of eight waves\): removed; "
                                  r"the default runs four windows per workgroup in teams of four waves, plan_flags\[2\] = 2 the same kernel with one",
    ("eqtransformer", (0, 0, 0, 1)): r"plan_flags\[3\] = 1 \(half-width decoder tiles\): removed; decoder.3 .. .6 run on the full-width tiles",
    ("eqtransformer", (0, 0, 0, 0, 0, 0, 0, 8192)): r"plan_flags\[7\] bit 13 \(ResCNN kernel with two windows per workgroup\): removed; "
                                                    r"the default runs three windows per workgroup \(eqt_res3t_kernel\), bit 9 one",
}


@pytest.mark.parametrize("name,flags", [(n, f) for n, fl in REMOVED_SELECTORS.items() for f in fl],
                         ids=[f"{n}-{'.'.join(map(str, f))}" for n, fl in REMOVED_SELECTORS.items() for f in fl])
def test_removed_plan_selectors_are_rejected(name, flags):
    from volpick_amd._lib import VolpickHipError

    m = MODELS[name].from_pretrained("volpick")
    m._plan_flags = flags
    with pytest.raises(VolpickHipError, match=REMOVED_MATCH.get((name, flags), "removed in round 6")):
        m.cuda()
        m(torch.zeros((1, 3, m.in_samples)).cuda())


# EQTransformer's layer dumps (plan_flags[1] & 4) exist for the default conv kernels only: every selector that swaps one out is refused
EQT_DUMP_REFUSED = [(1, 4), (0, 4, 0, 1), (0, 4, 0, 0, 0, 0, 2), (0, 4, 1), (0, 4, 2), (0, 4, 3)] + \
                   [(0, 4, 0, 0, 0, 0, 0, 1 << b) for b in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13)]


@pytest.mark.parametrize("flags", EQT_DUMP_REFUSED, ids=[".".join(map(str, f)) for f in EQT_DUMP_REFUSED])
def test_eqt_dumps_refuse_other_kernel_forms(flags):
    from volpick_amd._lib import VolpickHipError

    m = va.EQTransformer.from_pretrained("volpick")
    m._plan_flags = flags
    try:
        with pytest.raises(VolpickHipError, match="dumps the default conv kernels only"):
            m.cuda()
            m(torch.zeros((1, 3, m.in_samples)).cuda())
    finally:
        m._release()


@pytest.mark.parametrize("name,flags", [(n, f) for n, fl in PLAN_SELECTORS.items() for f in fl],
                         ids=[f"{n}-{'.'.join(map(str, f))}" for n, fl in PLAN_SELECTORS.items() for f in fl])
def test_every_plan_selector_is_oracle_grade(name, flags):
    oracle = load_pretrained(name, "volpick")
    m = MODELS[name].from_pretrained("volpick")
    m._plan_flags = flags
    m.cuda()
    try:
        x = synthetic_windows(3, m.in_samples, seed=4700)
        xn = OP.batch_pre(oracle, torch.from_numpy(x))
        with torch.no_grad():
            want = _as_array(oracle(xn))
        _check(_as_array(m(xn.cuda())), want, f"{name} plan_flags {flags}")
        got = _as_array(m._forward_raw(torch.from_numpy(x).cuda(), preprocess=True))  # the in-kernel / gather_normalize front end
        _check(got, want, f"{name} plan_flags {flags}, preprocessing on the device")
    finally:
        m._release()
