"""GPU: the pick-branch scope of EQTransformer's decoder trainer (volpick_amd/csrc/train_eqt_pick.hip,
``EQTransformerDecoderTrainer(scope="pick_branches")``).

Every kernel is checked from the values it read (``tensors()``, ``weights()``) against the float64 pieces of
tests/eqt_pick_restate.py at the bars that module's header counts; ``gradients()`` of all 66 tensors against float64 autograd
of the oracle's modules fed the device's ``pick.x`` and ``decoder.in[0]``, at four times the worst per-tensor distance of the
same computation in fp32 on the CPU (both normalised by the tensor's max |g|), computed here.  The tests print what they
measure; LOG.md records it.

Batch sizes: the network's lengths are fixed (47 steps), one workgroup serves one (branch, window) in every kernel and the fold
sums the windows one by one, so nothing tiles the batch: B in {1, 2, 3, 5} with max_batch = 8, and B = 4 = max_batch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import eqt_dec_restate as RD
from tests import eqt_pick_restate as R
from tests import train_state_f64 as TS
from tests.eqt_pick_restate import DROP, SEED, SIX_SIGMA
from tests.test_gpu_eqt_dec_train import FORWARD_BAR, W, bits, eqt_bank, make_batch, same_bits, wavelet_batch
from volpick_amd import EQTransformer, _lib
from volpick_amd import generate as G
from volpick_amd.train import EQTransformerDecoderTrainer, EQTransformerLit, decoder_param_names

pytestmark = pytest.mark.gpu
VP_ERR_INVALID = -1
U = RD.U


def trainer(name="volpick", max_batch=8, scope="pick_branches", drop_rate=DROP, seed=SEED, state=None, **kw):
    model = EQTransformer.from_pretrained(name)
    if state is not None:
        model.load_state_dict(state)
    return EQTransformerDecoderTrainer(model, max_batch=max_batch, scope=scope, drop_rate=drop_rate, seed=seed, **kw)


def branch(w, k):
    return R.branch_weights(w, k)


# ---- every kernel from the values it read ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, max_batch", [(1, 8), (2, 8), (3, 8), (5, 8), (4, 4)])
def test_every_pick_kernel_from_the_values_it_read(B, max_batch):
    tr = trainer(max_batch=max_batch)
    x, y = make_batch(B, seed=10 + B, zero_row=B == 3)
    tr.step(x, y, 0.0, W, update=False)  # step 0: discarded, so that the checked step is not the first
    loss = tr.step(x, y, 0.0, W, update=False)
    t, w, g = tr.tensors(B), tr.weights(), tr.gradients()
    assert np.isfinite(loss) and t["pick.x"].shape == (B, 16, 47) and t["pick.pre"].shape == (2, B, 64, 47)
    assert np.array_equal(t["pick.x"], t["decoder.in"][0])
    masks = R.mask(SEED, 1, B, DROP)
    assert np.array_equal(t["pick.mask"], masks)  # bit for bit the numpy Philox restatement
    r = {}

    def see(key, got, want, bar):
        r[key] = max(r.get(key, 0), TS.ratio(got, want, bar))

    for k in range(2):
        wk = branch(w, k)
        d = {n[5:]: a[k] for n, a in t.items() if n.startswith("pick.") and n != "pick.x"}
        # forward
        pre, abs_pre = R.pre_activations(t["pick.x"], d["h"], wk)
        see("pre", d["pre"], pre, RD.gamma(34) * abs_pre)
        act = R.gates(d["pre"])
        sig = np.ones(64, bool)
        sig[32:48] = False
        see("sigmoid", d["act"][:, sig], act[:, sig], 5 * U * act[:, sig] + RD.FLOOR)
        see("tanh", d["act"][:, ~sig], act[:, ~sig], R.TANH_U)
        c, abs_c = R.cell(d["act"], np.concatenate([np.zeros((B, 16, 1)), d["c"][..., :-1]], -1))
        see("c", d["c"], c, RD.gamma(3) * abs_c + RD.FLOOR)
        h = R.hidden(d["act"], d["c"])
        see("h", d["h"], h, np.abs(d["act"][:, 48:]) * R.TANH_U + 2 * U * np.abs(h) + RD.FLOOR)
        assert np.array_equal(d["hd"], R.dropped(d["h"], masks[k], DROP))  # exact given the mask and the float scale
        q, kk, abs_q, abs_k = R.qk(d["hd"], wk)
        see("q, k", d["q"], q, RD.gamma(17) * abs_q + RD.FLOOR)
        see("q, k", d["k"], kk, RD.gamma(17) * abs_k + RD.FLOOR)
        e, sum_wa, abs_e = R.scores(d["q"], d["k"], wk)
        see("scores", d["e"], e, 7 * U * sum_wa + RD.gamma(34) * abs_e)
        a, arg, dmax = R.weights_of(d["e"])
        assert np.array_equal(d["argmax"][:, 0], arg.astype(np.float32))  # the device's own scores, torch's tie rule
        see("a", d["a"], a, a * U * (12 + 2 * dmax) + RD.FLOOR)
        assert not d["a"][:, ~R.band()].any()
        v, abs_v = R.context(d["a"], d["hd"])
        see("v", d["v"], v, RD.gamma(3) * abs_v + RD.FLOOR)
        assert np.array_equal(t["decoder.in"][1 + k], d["v"])
        # backward
        wn = f"{RD.DEC_PREFIX[1 + k]}.convs.0.weight"
        bk0 = RD.stage_backward(t["decoder.in"][1 + k], t["a0"][1 + k], t["ga0"][1 + k], w[wn], RD.DOUT[0])
        see("gv", d["gv"], bk0["ga_in"], RD.gamma(RD.DCO[0] * RD.DK[0] + 1) * bk0["abs_ga_in"] + RD.FLOOR)
        bk = R.attention_backward(d["gv"], d["hd"], d["q"], d["k"], d["a"], d["argmax"][:, 0], wk)
        for n in ("gq", "gk", "ghd"):
            see("ghd, gq, gk", d[n], bk[n], RD.gamma(R.N_ATT) * bk["abs_" + n] + RD.FLOOR)
        assert np.array_equal(d["gh"], R.dropped(d["ghd"], masks[k], DROP))
        st = R.lstm_backward_steps(d["gh"], d["gpre"], d["gc"], d["act"], d["c"], wk["weight_hh_l0"])
        see("gpre", d["gpre"], st["gpre"], RD.gamma(R.N_LSTM) * st["abs_gpre"] + RD.FLOOR)
        see("gc", d["gc"], st["gc"], RD.gamma(R.N_LSTM) * st["abs_gc"] + RD.FLOOR)
        # the eighteen weight gradients from gpre, x, h, hd, gq, gk (and the recomputed score terms)
        lw = R.lstm_weight_grads(d["gpre"], t["pick.x"], d["h"])
        for n, key in zip(R.LSTM_KEYS, ("weight_ih_l0", "weight_hh_l0", "bias", "bias")):
            see("LSTM weights", g[f"pick_lstms.{k}.{n}"], lw[key], RD.gamma(47 * B + 2) * lw["abs_" + key] + RD.FLOOR)
        for n in ("Wx", "Wt", "bh", "Wa"):
            see("attention weights", g[f"pick_attentions.{k}.{n}"], bk[n].reshape(g[f"pick_attentions.{k}.{n}"].shape),
                RD.gamma(100 + 188 * B) * bk["abs_" + n].reshape(g[f"pick_attentions.{k}.{n}"].shape) + RD.FLOOR)
        ba = g[f"pick_attentions.{k}.ba"]
        assert ba[0] == 0.0 and not np.signbit(ba[0])
    print(f"B={B}: worst error / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(v <= 1 for v in r.values()), r
    tr.close()


# ---- end to end against autograd -------------------------------------------------------------------------------------------------
def autograd_66(w, x_pick, dec_in0, y, dtype):
    """(loss, gradients of the 66 tensors) of the oracle's modules: both branches (no dropout) into the three decoders."""
    nets = [R.build_branch(w, k, dtype) for k in range(2)]
    dec = RD.build(w, dtype)
    xt = torch.as_tensor(np.asarray(x_pick)).to(dtype)
    din = torch.stack([torch.as_tensor(np.asarray(dec_in0)).to(dtype)] + [n(xt)[2] for n in nets])
    loss = RD.loss_of(dec, din, torch.as_tensor(np.asarray(y)).to(dtype), W)
    loss.backward()
    grads = {k: p.grad.numpy().astype(np.float64) for k, p in dec.named_parameters()}
    for k, n in enumerate(nets):
        for name, p in n.named_parameters():
            mod, short = name.split(".", 1)
            grads[f"{'pick_lstms' if mod == 'lstm' else 'pick_attentions'}.{k}.{short}"] = p.grad.numpy().astype(np.float64)
    return float(loss.detach()), grads


def edited_state(name, edits):
    sd = EQTransformer.from_pretrained(name).state_dict()
    for n, f in edits.items():
        sd[n] = sd[n] * np.float32(f)
    return sd


@pytest.mark.parametrize("name, B, edits", [("volpick", 2, None), ("volpick_95train", 3, None),
                                            ("volpick", 2, {"pick_attentions.0.Wa": 200.0}),
                                            ("volpick", 2, {"pick_attentions.1.Wa": 0.0})])
def test_gradients_of_the_66_tensors_against_float64_autograd(name, B, edits):
    """The third case: a row maximum outside the band in most rows of the P branch (tests/test_eqt_pick_train_cpu.py shows
    that a backward without the argmax path misses this bar on that case).  The fourth: every score of the S branch equals
    ba, each row's maximum is attained 47 times and the kept argmax must be column 0, torch's choice; Wx, Wt and bh of that
    branch then have no gradient at all."""
    tr = trainer(name, drop_rate=0.0, state=None if edits is None else edited_state(name, edits))
    x, y = make_batch(B, seed=20 + B, zero_row=True)
    loss = tr.step(x, y, 0.0, W, update=False)
    t, w, g = tr.tensors(B), tr.weights(), tr.gradients()
    assert t["pick.mask"].all()
    if edits == {"pick_attentions.0.Wa": 200.0}:
        outside = np.abs(t["pick.argmax"][0, :, 0] - np.arange(47)) > 1
        assert outside.mean() > 0.5
    if edits == {"pick_attentions.1.Wa": 0.0}:
        assert (t["pick.e"][1] == w["pick_attentions.1.ba"][0]).all() and (t["pick.argmax"][1] == 0).all()
    loss64, g64 = autograd_66(w, t["pick.x"], t["decoder.in"][0], y, torch.float64)
    loss32, g32 = autograd_66(w, t["pick.x"], t["decoder.in"][0], y, torch.float32)
    ba = [k for k in g64 if k.endswith(".ba")]
    for k in ba:  # zero in exact arithmetic: float64 leaves rounding noise, the device writes +0.0
        assert g[k][0] == 0.0 and abs(g64[k][0]) <= 1e-12 * np.abs(g64[k.replace(".ba", ".Wa")]).max()
    none = [k for k in g64 if k not in ba and not g64[k].any()]  # (the tied case: exact zeros on both sides)
    assert all(not g[k].any() for k in none) and len(none) == (3 if edits == {"pick_attentions.1.Wa": 0.0} else 0), none
    keys = [k for k in g64 if k not in ba and k not in none]
    dist = lambda got: {k: float(np.abs(np.asarray(got[k], np.float64) - g64[k]).max() / np.abs(g64[k]).max()) for k in keys}
    dev, cpu = dist(g), dist(g32)
    bar = 4 * max(cpu.values())
    k_dev, k_cpu = max(dev, key=dev.get), max(cpu, key=cpu.get)
    pick = [k for k in keys if R.is_pick_key(k)]
    print(f"{name} B={B} edits={edits}: loss {loss:.9g} (float64 {loss64:.9g}); worst distance / max|g|: device {dev[k_dev]:.3g} "
          f"({k_dev}), fp32 CPU {cpu[k_cpu]:.3g} ({k_cpu}); bar {bar:.3g}; pick tensors: device {max(dev[k] for k in pick):.3g}, "
          f"fp32 CPU {max(cpu[k] for k in pick):.3g}")
    assert len(keys) + len(none) == 64 and len(g) == 66
    assert abs(loss - loss64) <= 1e-6 * abs(loss64)
    assert max(dev.values()) <= bar, (dev[k_dev], k_dev, bar)
    tr.close()


def test_ba_keeps_its_bits_through_three_updates():
    tr = trainer()
    x, y = make_batch(2, seed=27)
    w0 = tr.weights()
    for _ in range(3):
        tr.step(x, y, 1e-3, W)
    w1 = tr.weights()
    for k in range(2):
        assert (bits(w0[f"pick_attentions.{k}.ba"]) == bits(w1[f"pick_attentions.{k}.ba"])).all()
        assert (bits(w0[f"pick_attentions.{k}.Wa"]) != bits(w1[f"pick_attentions.{k}.Wa"])).any()
    tr.close()


# ---- forward against inference, scopes side by side -------------------------------------------------------------------------------
def test_forward_without_dropout_is_the_inference_forward_and_scope_0_is_untouched():
    B = 3
    x, y = make_batch(B, seed=35)
    a = trainer(scope="decoders")
    b = trainer(scope="pick_branches", drop_rate=0.0)
    la, lb = a.step(x, y, 0.0, W, update=False), b.step(x, y, 0.0, W, update=False)
    ta, tb, ga, gb = a.tensors(B), b.tensors(B), a.gradients(), b.gradients()
    # scope 0's decoder.in is the inference plan's: the training forward of the branches agrees with it at the forward bar
    err = np.abs(tb["decoder.in"][1:] - ta["decoder.in"][1:]).max()
    print(f"max |training forward - inference| of decoder.in[1:] = {err:.3g}")
    assert err <= FORWARD_BAR and err > 0
    # set 0 -- the detection decoder -- does not see the branches: tensors and gradients bit-equal between the scopes
    for k in ta:
        if k == "p":
            assert (bits(ta[k][:, 0]) == bits(tb[k][:, 0])).all(), k
        else:
            assert (bits(ta[k][0]) == bits(tb[k][0])).all(), k
    for k in ga:
        if k.startswith(("decoder_d.", "conv_d.")):
            assert (bits(ga[k]) == bits(gb[k])).all(), k
    assert not any(k.startswith("pick.") for k in ta) and len(ga) == 48 and len(gb) == 66
    assert b.launch_count() == a.launch_count() + 7  # two forward, stage 0's input gradient, two adjoints, weight gradient, fold
    # a scope-0 trainer made through create_scope is the trainer of create: same bits everywhere, same launches
    lib = _lib.load()
    model = EQTransformer.from_pretrained("volpick")
    wts = np.ascontiguousarray(model._weights, np.float32)
    cfg = model._config()
    h = C.c_void_p()
    assert lib.vp_eqt_dec_train_create(0, _lib.ptr(wts), wts.size, C.byref(cfg), 8, C.byref(h)) == 0
    try:
        assert lib.vp_eqt_dec_train_scope(h) == 0 and lib.vp_eqt_dec_train_scope(a._h) == 0 and lib.vp_eqt_dec_train_scope(b._h) == 1
        loss = C.c_double()
        wd = (C.c_double * 3)(*W)
        assert lib.vp_eqt_dec_train_step(h, _lib.ptr(x), _lib.ptr(y), _lib.VP_MEM_HOST, B, wd, 0.0, 0, C.byref(loss)) == 0
        assert loss.value == la and lib.vp_eqt_dec_train_launch_count(h) == a.launch_count()
        n = lib.vp_eqt_dec_train_weight_count()
        for which in (0, 1):
            got = np.empty(n, np.float32)
            assert lib.vp_eqt_dec_train_read(h, which, _lib.ptr(got), n) == 0
            assert (bits(got) == bits(a._read(which))).all()
        assert lib.vp_eqt_dec_train_tensor_count(h) == lib.vp_eqt_dec_train_tensor_count(a._h)
        for i in range(lib.vp_eqt_dec_train_tensor_count(h)):
            name, s, c, l = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
            assert lib.vp_eqt_dec_train_tensor_info(h, i, C.byref(name), C.byref(s), C.byref(c), C.byref(l)) == 0
            got = np.empty((s.value, B, c.value, l.value), np.float32)
            assert lib.vp_eqt_dec_train_tensor_read(h, i, B, _lib.ptr(got)) == 0
            want = ta[name.value.decode()]
            assert (bits(got.reshape(want.shape)) == bits(want)).all(), name.value
    finally:
        lib.vp_eqt_dec_train_destroy(h)
    a.close(), b.close()


# ---- determinism and state ---------------------------------------------------------------------------------------------------------
def test_two_trainers_hold_the_same_bits_and_the_seed_sets_the_masks():
    a, b, c = trainer(), trainer(), trainer(seed=SEED + 1)
    batches = [make_batch(B, seed=40 + i, zero_row=i == 2) for i, B in enumerate((2, 5, 1))]
    for tr in (a, b, c):
        tr.losses = [tr.step(x, y, 1e-3, W) for x, y in batches]
    assert a.losses == b.losses and same_bits(a.weights(), b.weights()) and same_bits(a.gradients(), b.gradients())
    assert all(same_bits(s, t) for s, t in zip(a.adam_state(), b.adam_state()))
    ta, tb, tc = a.tensors(1), b.tensors(1), c.tensors(1)
    assert all((bits(ta[k]) == bits(tb[k])).all() for k in ta)
    assert not np.array_equal(ta["pick.mask"], tc["pick.mask"]) and a.losses != c.losses
    # a step with update = False advances the count all the same: the next mask is step 4's, not step 3's again
    x, y = make_batch(8, seed=44)
    a.step(x, y, 0.0, W, update=False)
    m3 = a.tensors(8)["pick.mask"]
    a.step(x, y, 0.0, W, update=False)
    m4 = a.tensors(8)["pick.mask"]
    assert np.array_equal(m3, R.mask(SEED, 3, 8, DROP)) and np.array_equal(m4, R.mask(SEED, 4, 8, DROP)) and a.global_step == 3
    assert abs(m3.mean() - 0.9) <= SIX_SIGMA and abs(m4.mean() - 0.9) <= SIX_SIGMA
    # export: the 66 tensors move, every other tensor keeps its bits
    start = EQTransformer.from_pretrained("volpick").state_dict()
    after, trained = a.export().state_dict(), a.weights()
    names = {k for k, _ in a.names}
    assert len(names) == 66 and list(after) == list(start)
    for k in after:
        if k in names:
            assert (bits(after[k]) == bits(trained[k])).all(), k
            assert k.endswith(".ba") or not (bits(after[k]) == bits(start[k])).all(), k
        else:
            assert np.array_equal(after[k], start[k]) and after[k].dtype == start[k].dtype, k
    a.close(), b.close(), c.close()


def test_blobs_have_the_handles_size_and_bad_drop_rates_are_refused():
    lib = _lib.load()
    tr = trainer(max_batch=4)
    w0 = tr.weights()
    blob = np.concatenate([w0[k].ravel() for k, _ in tr.names])
    assert blob.size == 152261 == tr.n_params
    tr.write_weights(blob[::-1].copy())
    assert (bits(tr._read(0)) == bits(blob[::-1])).all()
    tr.write_weights(w0)  # a dict of the 66 tensors
    assert same_bits(tr.weights(), w0)
    small = np.zeros(145731, np.float32)
    assert lib.vp_eqt_dec_train_write_weights(tr._h, _lib.ptr(small), small.size) == VP_ERR_INVALID
    assert b"152261" in lib.vp_last_error()
    assert lib.vp_eqt_dec_train_read(tr._h, 0, _lib.ptr(small), small.size) == VP_ERR_INVALID and b"bad size" in lib.vp_last_error()
    with pytest.raises(ValueError, match="flat blob of 152261"):
        tr.write_weights(small)
    assert same_bits(tr.weights(), w0)
    dec = trainer(scope="decoders", max_batch=4)
    assert dec.n_params == 145731 and [k for k, _ in dec.names] == [k for k, _ in decoder_param_names()]
    with pytest.raises(_lib.VolpickHipError, match="pick_ms"):
        dec.pick_ms()
    dec.close(), tr.close()
    for bad in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(_lib.VolpickHipError, match="drop_rate"):
            trainer(drop_rate=bad, max_batch=2)
    model = EQTransformer.from_pretrained("volpick")
    wts, cfg, h = np.ascontiguousarray(model._weights, np.float32), model._config(), C.c_void_p()
    assert lib.vp_eqt_dec_train_create_scope(0, _lib.ptr(wts), wts.size, C.byref(cfg), 2, 2, 0.1, 0, C.byref(h)) == VP_ERR_INVALID
    assert not h.value


# ---- it trains ---------------------------------------------------------------------------------------------------------------------
def test_three_adam_steps_follow_the_float64_oracle_extended_to_the_66_tensors():
    """tests/test_gpu_eqt_dec_train.py's check of the loss ratio (bar 0.01), three steps, no dropout."""
    tr = trainer(drop_rate=0.0)
    x, y = wavelet_batch()
    first = tr.step(x, y, 0.0, W, update=False)
    t, w = tr.tensors(4), tr.weights()
    nets = [R.build_branch(w, k) for k in range(2)]
    dec = RD.build(w)
    params = [p for n in nets + [dec] for p in n.parameters()]
    opt = torch.optim.Adam(params, lr=1e-3)
    xt, d0, yt = (torch.as_tensor(np.asarray(v)).double() for v in (t["pick.x"], t["decoder.in"][0], y))
    oracle = []
    for _ in range(3):
        opt.zero_grad()
        loss = RD.loss_of(dec, torch.stack([d0] + [n(xt)[2] for n in nets]), yt, W)
        loss.backward()
        opt.step()
        oracle.append(float(loss.detach()))
    losses = [tr.step(x, y, 1e-3, W) for _ in range(3)]
    ratio, want = losses[2] / losses[0], oracle[2] / oracle[0]
    print(f"loss {losses[0]:.6g} -> {losses[2]:.6g} (ratio {ratio:.5f}); float64 oracle {oracle[0]:.6g} -> {oracle[2]:.6g} ({want:.5f})")
    assert losses[0] == first and abs(losses[0] - oracle[0]) <= 1e-6 * oracle[0]
    assert oracle[2] < oracle[0] and abs(ratio - want) <= 0.01
    w3 = tr.weights()
    want_w = {f"pick_lstms.{k}.weight_hh_l0": n.lstm.weight_hh_l0 for k, n in enumerate(nets)}
    want_w.update({f"pick_attentions.{k}.Wt": n.att.Wt for k, n in enumerate(nets)})
    for k, p in want_w.items():  # each element moved by about 3 lr; the device's follows the oracle's to a tenth of a step
        assert np.abs(w3[k] - p.detach().numpy()).max() <= 1e-4 and np.abs(w3[k] - w[k]).max() > 1e-3, k
    tr.close()


@pytest.fixture(scope="module")
def bank():
    b = eqt_bank()
    yield b
    b.close()


def test_the_lit_fits_the_pick_branches_and_keeps_the_best_66(bank):
    start = EQTransformer.from_pretrained("volpick")
    lit = EQTransformerLit(lr=1e-2, sigma=20, model=EQTransformer.from_pretrained("volpick"), trainable="pick_branches", max_batch=8,
                           seed=SEED)
    n = bank.n_traces
    train = G.WaveformBank([bank.trace(i) for i in range(16)], {"P": bank.onsets[:16, :2], "S": bank.onsets[:16, 2:]})
    val = G.WaveformBank([bank.trace(i) for i in range(16, n)], {"P": bank.onsets[16:, :2], "S": bank.onsets[16:, 2:]})
    try:
        losses, val_losses = lit.fit_bank(train, 4, batch_size=8, seed=1, val_bank=val, keep_best=True)
        tr = lit.trainer_state
        assert tr.scope == "pick_branches" and tr.drop_rate == 0.1 and tr.seed == SEED
        assert len(losses) == 4 and len(val_losses) == 2 and np.isfinite(losses).all() and np.isfinite(val_losses).all()
        assert tr.global_step == 4 and set(lit.best_state) == {k for k, _ in tr.names} and len(lit.best_state) == 66
        assert same_bits(tr.weights(), lit.best_state)
        sd, sd0 = lit.model.state_dict(), start.state_dict()
        assert all((bits(sd[k]) == bits(lit.best_state[k])).all() for k in lit.best_state)
        for k in sd:  # the detection trunk (and everything else outside the 66) keeps its bits
            if k not in lit.best_state:
                assert np.array_equal(sd[k], sd0[k]), k
        assert any((bits(sd[k]) != bits(sd0[k])).any() for k in sd if R.is_pick_key(k))
        xb = torch.from_numpy(make_batch(2, seed=55)[0]).cuda()
        new, old = lit.model.cuda()(xb), start.cuda()(xb)
        assert not torch.equal(new[1], old[1]) and not torch.equal(new[2], old[2])  # P and S outputs differ
        assert torch.isfinite(torch.stack(new)).all()
    finally:
        train.close(), val.close()
        lit.trainer_state.close()
