"""CPU: the surface of the pick-branch training scope (vp_eqt_dec_train_*scope*, EQTransformerDecoderTrainer(scope=...),
EQTransformerLit(trainable="pick_branches")) and the numpy restatement of tests/eqt_pick_restate.py against float64 autograd of
the oracle's own nn.LSTM and _SeqSelfAttention: on the released weights, on weights edited so that a row's maximum lies outside
its band or is attained twice, with the planted fault the GPU bars must see, and the dropout masks."""
import copy
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.models import load_pretrained
from tests import eqt_dec_restate as RD
from tests import eqt_pick_restate as R
from volpick_amd import EQTransformer, _lib
from volpick_amd import train as TR
from volpick_amd.synthetic import synthetic_windows

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("create_scope", "scope", "scope_param_count", "scope_param_name", "scope_param_size", "scope_weight_count", "pick_ms")
DROP, SEED, SIX_SIGMA = R.DROP, R.SEED, R.SIX_SIGMA


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_and_bound(lib):
    hdr = (ROOT / "include" / "volpick_hip.h").read_text()
    for short in NEW_SYMBOLS:
        name = "vp_eqt_dec_train_" + short
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
        assert decl, f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        n_args = 0 if decl.group(1).strip() == "void" else decl.group(1).count(",") + 1
        assert len(argtypes) == n_args, name
    assert re.search(r"VP_EQT_TRAIN_DECODERS = 0, VP_EQT_TRAIN_PICK_BRANCHES = 1", hdr)
    assert TR.TRAIN_SCOPES == {"decoders": 0, "pick_branches": 1}


def test_the_66_tensors_are_the_blob_tables_rows_with_the_four_prefixes_in_its_order(lib):
    kind = _lib.VP_MODEL_EQTRANSFORMER
    table = [(lib.vp_param_name(kind, i).decode(), int(lib.vp_param_size(kind, i))) for i in range(lib.vp_param_count(kind))]
    want = [(k, n) for k, n in table if RD.is_decoder_key(k) or R.is_pick_key(k)]
    got = TR.pick_branch_param_names()
    assert got == want and len(got) == 66 == lib.vp_eqt_dec_train_scope_param_count(1)
    assert sum(n for _, n in got) == R.N_FLOATS == lib.vp_eqt_dec_train_scope_weight_count(1) == 152261
    sizes = dict(got)
    for k in range(2):
        for n, size in zip(R.LSTM_KEYS, (1024, 1024, 64, 64)):
            assert sizes[f"pick_lstms.{k}.{n}"] == size
        for n, size in zip(R.ATT_KEYS, (512, 512, 32, 32, 1)):
            assert sizes[f"pick_attentions.{k}.{n}"] == size
    assert sum(n for k, n in got if R.is_pick_key(k)) == 6530 and sum(1 for k, _ in got if R.is_pick_key(k)) == 18
    # scope 0 through the new entries is the old list; the old entries keep their answers
    old = [(lib.vp_eqt_dec_train_scope_param_name(0, i).decode(), int(lib.vp_eqt_dec_train_scope_param_size(0, i)))
           for i in range(lib.vp_eqt_dec_train_scope_param_count(0))]
    assert old == TR.decoder_param_names() and len(old) == 48 == lib.vp_eqt_dec_train_param_count()
    assert lib.vp_eqt_dec_train_weight_count() == lib.vp_eqt_dec_train_scope_weight_count(0) == 145731
    assert lib.vp_eqt_dec_train_scope_param_name(1, 66) is None and lib.vp_eqt_dec_train_scope_param_size(1, -1) == 0
    for bad in (-1, 2):
        assert lib.vp_eqt_dec_train_scope_param_count(bad) == 0 and lib.vp_eqt_dec_train_scope_weight_count(bad) == 0
        assert lib.vp_eqt_dec_train_scope_param_name(bad, 0) is None


def test_trainable_accepts_pick_branches_and_still_refuses_the_rest():
    model = object.__new__(TR.EQTransformer)
    model.in_samples = 6000
    assert TR.TRAINABLE == ("decoders", "pick_branches")
    lit = TR.EQTransformerLit(model=model, trainable="pick_branches", drop_rate=0.2, seed=5)
    assert lit.trainable == "pick_branches" and lit._trainer is None and (lit.drop_rate, lit.seed) == (0.2, 5)
    assert TR.EQTransformerLit(model=model, trainable="pick_branches").drop_rate is None  # SeisBench's 0.1, set by the trainer
    assert TR.EQT_DROP_RATE == 0.1
    for bad in ("all", "trunk", "decoder", True, 1):
        with pytest.raises(ValueError, match="'decoders'"):
            TR.EQTransformerLit(model=model, trainable=bad)
    with pytest.raises(NotImplementedError, match="trainable='decoders'"):
        TR.EQTransformerLit(model=model).training_step({"X": None, "y": None, "detections": None})
    with pytest.raises(ValueError, match="scope must be one of"):
        TR.EQTransformerDecoderTrainer(EQTransformer.from_pretrained("volpick"), scope="trunk")


# ---- the restatement against float64 autograd ---------------------------------------------------------------------------------------
def oracle_and_state(name, edits=None):
    """(oracle network in float64, state dict for the library's model) with the tensors named in ``edits`` multiplied."""
    net = copy.deepcopy(load_pretrained("eqtransformer", name))
    sd = EQTransformer.from_pretrained(name).state_dict()
    params = dict(net.named_parameters())
    with torch.no_grad():
        for n, f in (edits or {}).items():
            params[n].mul_(f)
            sd[n] = sd[n] * np.float32(f)
    return net.double().eval(), {k: np.asarray(v) for k, v in sd.items()}


def bottleneck(net, B, seed):
    x = synthetic_windows(B, 6000, seed=seed).astype(np.float64)
    x -= x.mean(-1, keepdims=True)
    x /= np.abs(x).max((1, 2), keepdims=True)
    with torch.no_grad():
        return net.bottleneck(torch.from_numpy(x)).numpy()


def within(got, want, terms, what):
    bar = R.CPU_BAR * np.asarray(terms, np.float64) + 1e-300
    worst = float((np.abs(np.asarray(got) - want) / bar).max())
    assert worst <= 1, (what, worst)


def compare_branch(state, k, x, gv, m, drop):
    """restatement against autograd, everything it shares; returns both."""
    sc = float(R.scale_of(drop))
    auto = R.branch_autograd(state, k, x, gv, m, sc)
    mine = R.restated_gradients(state, k, x, gv, m, drop)
    within(mine["h"], auto["h"], R.CHAIN, "h")  # (R.CHAIN: the restatement's header)
    within(mine["hd"], auto["hd"], R.CHAIN, "hd")
    within(mine["v"], auto["v"], R.CHAIN * (1 + np.abs(auto["v"])), "v")
    for key in ("ghd", "Wx", "Wt", "bh", "Wa"):
        within(mine[key], auto[key].reshape(mine[key].shape), mine["abs_" + key], key)
    scale = np.abs(auto["gh"]).max()
    within(mine["gh"], auto["gh"], 2 * mine["abs_ghd"] * sc + scale, "gh")
    for key in R.LSTM_KEYS:
        within(mine[key], auto[key], R.CHAIN * mine["abs_" + key], key)
    assert mine["ba"][0] == 0.0 and abs(auto["ba"][0]) <= 1e-12 * max(np.abs(auto["bh"]).max(), np.abs(auto["Wa"]).max())
    return mine, auto


@pytest.mark.parametrize("name, B", [("volpick", 2), ("volpick_95train", 3)])
def test_the_restatement_equals_float64_autograd_on_the_released_weights(name, B):
    net, state = oracle_and_state(name)
    x = bottleneck(net, B, seed=70 + B)
    rng = np.random.default_rng(B)
    masks = R.mask(SEED, 3, B, DROP)
    for k in range(2):
        gv = rng.standard_normal((B, 16, R.T)) * 1e-3
        # dropout on: the mask and the float scale enter forward and backward
        mine, _ = compare_branch(state, k, x, gv, masks[k], DROP)
        assert 0 < (mine["hd"] == 0).mean() < 0.3
        # dropout off is the oracle's eval-mode function: its own forward gives the same v
        mine, _ = compare_branch(state, k, x, gv, None, 0.0)
        with torch.no_grad():
            px = net.pick_lstms[k](torch.from_numpy(x).permute(2, 0, 1))[0].permute(1, 2, 0)
            v = net.pick_attentions[k](px)[0].numpy()
        within(mine["v"], v, R.CHAIN * (1 + np.abs(v)), "v of the oracle's branch")
        # on these weights every row's maximum lies in its band or next to it, and the maximum's share is small but present
        share = 1 - mine["a"].sum(-1)
        assert 0 < share.min() and share.max() < 1e-3


def test_one_lstm_step_and_its_adjoint_equal_autograd_of_nn_lstm():
    net, state = oracle_and_state("volpick")
    x = bottleneck(net, 2, seed=75)
    w = R.branch_weights(state, 1)
    fw = R.lstm_forward(x, w)
    t = 5
    rng = np.random.default_rng(9)
    gh, gc, gnext = rng.standard_normal((2, 16)), rng.standard_normal((2, 16)), rng.standard_normal((2, 64))
    lstm = R.build_branch(state, 1).lstm
    h0 = torch.tensor(fw["h"][:, :, t - 1], requires_grad=True)
    c0 = torch.tensor(fw["c"][:, :, t - 1], requires_grad=True)
    out, (h1, c1) = lstm(torch.from_numpy(x[:, :, t])[None], (h0[None], c0[None]))
    within(fw["h"][:, :, t], h1[0].detach().numpy(), R.CHAIN, "h_t")
    within(fw["c"][:, :, t], c1[0].detach().numpy(), R.CHAIN * (1 + np.abs(fw["c"][:, :, t])), "c_t")
    # h_t feeds the outside (gh) and step t + 1's pre-activation (W_hh^T gpre_{t+1}); c_t feeds step t + 1 (gc)
    loss = (h1[0] * torch.from_numpy(gh)).sum() + (c1[0] * torch.from_numpy(gc)).sum() \
        + ((h1[0] @ lstm.weight_hh_l0.T) * torch.from_numpy(gnext)).sum()
    g_c0, g_bias, g_wih = torch.autograd.grad(loss, [c0, lstm.bias_ih_l0, lstm.weight_ih_l0])
    st = R.lstm_step_backward(gh, gnext, gc, fw["act"][:, :, t], fw["c"][:, :, t], fw["c"][:, :, t - 1], w["weight_hh_l0"])
    within(st["gc_prev"], g_c0.numpy(), st["abs_gc_prev"], "gc_{t-1}")
    within(st["gpre"].sum(0), g_bias.numpy(), st["abs_gpre"].sum(0), "sum of gpre_t")
    within(np.einsum("br,bc->rc", st["gpre"], x[:, :, t]), g_wih.numpy(), np.einsum("br,bc->rc", st["abs_gpre"], np.abs(x[:, :, t])), "gpre_t x_t")


def fp32_bar(state, k, x, gv):
    """The GPU test's end-to-end bar for one branch: four times the worst distance of the oracle's modules run in fp32 from
    float64, normalised per tensor by max |g|; ba (zero) left out."""
    g64, g32 = R.branch_autograd(state, k, x, gv), R.branch_autograd(state, k, x, gv, dtype=torch.float32)
    keys = [n for n in R.LSTM_KEYS + R.ATT_KEYS if n != "ba"]
    return 4 * max(np.abs(g32[n] - g64[n]).max() / np.abs(g64[n]).max() for n in keys), g64, keys


def test_a_maximum_outside_the_band_and_the_fault_of_ignoring_it():
    """pick_attentions.0.Wa x 200 (tests/test_gpu_layers_f64.py's eps-dominated rows): the rows' maxima lie far outside their
    bands, and the gradient through the maximum is no longer small."""
    net, state = oracle_and_state("volpick", {"pick_attentions.0.Wa": 200.0})
    x = bottleneck(net, 2, seed=81)
    gv = np.random.default_rng(1).standard_normal((2, 16, R.T)) * 1e-3
    mine, auto = compare_branch(state, 0, x, gv, None, 0.0)
    i = np.arange(R.T)
    outside = np.abs(mine["argmax"] - i) > 1
    assert outside.mean() > 0.5, outside.mean()
    # the mutation: a backward that takes the row maximum for a constant misses autograd by more than the GPU test's bar
    bar, g64, keys = fp32_bar(state, 0, x, gv)
    wrong = R.restated_gradients(state, 0, x, gv, None, 0.0, argmax_path=False)
    dist = {n: np.abs(wrong[n].reshape(g64[n].shape) - g64[n]).max() / np.abs(g64[n]).max() for n in keys}
    right = {n: np.abs(mine[n].reshape(g64[n].shape) - g64[n]).max() / np.abs(g64[n]).max() for n in keys}
    print(f"bar {bar:.3g}; without the argmax path: " + ", ".join(f"{n} {v:.3g}" for n, v in dist.items()))
    assert max(right.values()) < 1e-9 and bar < 1e-3
    assert all(dist[n] > bar for n in ("Wa", "Wx", "Wt", "bh", "weight_ih_l0", "weight_hh_l0")), (dist, bar)


def test_two_equal_maxima_send_the_gradient_to_the_lower_index():
    """pick_attentions.1.Wa x 0: every score of a row equals ba, the maximum is attained 47 times and torch.max keeps column 0."""
    net, state = oracle_and_state("volpick", {"pick_attentions.1.Wa": 0.0})
    x = bottleneck(net, 2, seed=82)
    gv = np.random.default_rng(2).standard_normal((2, 16, R.T)) * 1e-3
    mine, auto = compare_branch(state, 1, x, gv, None, 0.0)
    assert (mine["argmax"] == 0).all() and np.abs(auto["Wa"]).max() > 0
    # with the maximum's share sent to the highest index instead, Wa's gradient is another one
    q, k = mine["q"], mine["k"]
    other = R.attention_backward(gv, mine["hd"], q, k, mine["a"], np.full((2, R.T), R.T - 1), R.branch_weights(state, 1))
    assert np.abs(other["Wa"] - auto["Wa"]).max() > 1e3 * R.CPU_BAR * mine["abs_Wa"].max()


# ---- dropout masks -------------------------------------------------------------------------------------------------------------------
def test_the_masks_of_the_gpu_tests_seed_keep_nine_tenths_and_never_repeat():
    assert SIX_SIGMA == pytest.approx(0.0164, abs=1e-4)
    for step in range(4):
        m = R.mask(SEED, step, 8, DROP)
        assert m.shape == (2, 8, 16, R.T) and set(np.unique(m)) == {0.0, 1.0}
        assert abs(m.mean() - 0.9) <= SIX_SIGMA, (step, m.mean())
        assert not np.array_equal(m, R.mask(SEED, step + 1, 8, DROP))  # steps n and n + 1
        assert not np.array_equal(m[0], m[1])  # the two branches
        assert not np.array_equal(m, R.mask(SEED + 1, step, 8, DROP))
        assert np.array_equal(m[:, :3], R.mask(SEED, step, 3, DROP))  # a window's mask does not depend on the batch size
    assert R.mask(SEED, 0, 8, 0.0).all()  # drop_rate 0 keeps everything, at scale exactly 1
    assert R.scale_of(0.0) == 1.0 and R.scale_of(0.1) == np.float32(1.0) / np.float32(0.9)
    h = np.random.default_rng(3).standard_normal((2, 8, 16, R.T)).astype(np.float32)
    hd = R.dropped(h, R.mask(SEED, 0, 8, DROP), DROP)
    assert hd.dtype == np.float32 and ((hd == 0) == (R.mask(SEED, 0, 8, DROP) == 0)).all()
