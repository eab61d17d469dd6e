"""The bars of tests/train_state_f64.py on the CPU: float32 emulations of adam_kernel, of the BatchNorm running statistics and
of the loss head stay inside them, and each wrong form a kernel or host path could take exceeds one -- so a GPU run that
passes tests/test_gpu_train_state.py cannot hide any of these."""
import numpy as np
import pytest

from tests import train_state_f64 as TS

ADAM_SETS = TS.HYPER_SETS + ((0.95, 0.9999, 1e-10, 0.1, 1e-5), (0.0, 0.25, 1e-8, 0.1, 1e-5))
LRS = (1e-3, 5e-4, 0.0, 2e-3, 1e-3, 1e-2)
N = 4096


def gradients(seed):
    """|g| log-uniform over 1e-12 .. 1e2, random signs (so that a carried moment meets opposing gradients), exact zeros."""
    rng = np.random.default_rng(seed)
    g = 10.0 ** rng.uniform(-12, 2, N) * rng.choice([-1.0, 1.0], N)
    g[rng.integers(0, N, N // 16)] = 0.0
    return g.astype(np.float32)


def adam_run(hyper, mutation=None, updates=(True,) * 6, count_every_launch=False):
    """The emulation over a run of steps (``updates``: which of them update), each update compared with adam_update on the
    state it read.  Returns the worst ratios (m, v, w, w against the plain bar) over the run."""
    b1, b2, eps = hyper[:3]
    rng = np.random.default_rng(1)
    w = rng.standard_normal(N).astype(np.float32)
    m = np.zeros(N, np.float32)
    v = np.zeros(N, np.float32)
    t = t_emulated = 0
    worst = np.zeros(4)
    for i, update in enumerate(updates):
        g = gradients(10 + i)
        if not update:
            t_emulated += int(count_every_launch)
            continue
        t, t_emulated = t + 1, t_emulated + 1
        lr = LRS[i % len(LRS)]
        ref = TS.adam_update(w, g, m, v, t, lr, b1, b2, eps)
        m1, v1, w1 = TS.adam_emulated(w, g, m, v, t_emulated, lr, b1, b2, eps, mutation)
        worst = np.maximum(worst, [TS.ratio(m1, ref.m, ref.bar_m), TS.ratio(v1, ref.v, ref.bar_v),
                                   TS.ratio(w1, ref.w, ref.bar_w), TS.ratio(w1, ref.w, ref.bar_w_plain)])
        if lr == 0.0:
            assert np.array_equal(w1, w)
        w, m, v = w1, m1, v1
    return worst


@pytest.mark.parametrize("hyper", ADAM_SETS)
def test_adam_emulation_stays_inside_the_bars(hyper):
    rm, rv, rw, plain = adam_run(hyper)
    print(f"\n{hyper}: worst got/bar m {rm:.3f} v {rv:.3f} w {rw:.3f} (w against the plain bar {plain:.3f})")
    assert rm <= 1.0 and rv <= 1.0 and rw <= 1.0


def test_a_cancelling_moment_misses_the_plain_weight_bar_and_holds_the_full_one():
    """m = 1 meets g = -9 (1 + d): m' = -0.9 d carries the roundings of two terms of size 0.9, a relative error of u / d."""
    d = 10.0 ** np.linspace(-6, -3, 512)
    g = (-9.0 * (1.0 + d)).astype(np.float32)
    m = np.ones_like(g)
    v = np.full_like(g, 50.0)
    w = np.zeros_like(g)  # (a weight of ordinary size hides it behind its own rounding, u |w'|)
    ref = TS.adam_update(w, g, m, v, 5, 1e-3, 0.9, 0.999, 1e-8)
    m1, v1, w1 = TS.adam_emulated(w, g, m, v, 5, 1e-3, 0.9, 0.999, 1e-8)
    assert TS.ratio(m1, ref.m, ref.bar_m) <= 1.0 and TS.ratio(w1, ref.w, ref.bar_w) <= 1.0
    assert TS.ratio(w1, ref.w, ref.bar_w_plain) > 1.0
    # an element that does not cancel has the plain bar, to rounding
    same = TS.adam_update(w, -g, m, v, 5, 1e-3, 0.9, 0.999, 1e-8)
    assert np.all(same.bar_w <= same.bar_w_plain * (1.0 + 1e-9))


@pytest.mark.parametrize("mutation,which,least", [
    ("count_off_by_one", 2, 1e3),
    ("bc2_without_root", 2, 1e3),
    ("eps_inside_root", 2, 1e4),
    ("default_eps", 2, 1.0),
    ("default_betas", 0, 1.0),
    ("default_betas", 1, 1.0),
])
def test_adam_mutations_exceed_the_bars(mutation, which, least):
    hyper = TS.HYPER_SETS[1] if mutation.startswith("default") else TS.DEFAULT_HYPER
    worst = adam_run(hyper, mutation)
    print(f"\n{mutation}: got/bar m {worst[0]:.3g} v {worst[1]:.3g} w {worst[2]:.3g}")
    assert worst[which] > least


def test_a_count_that_advances_without_an_update_exceeds_the_weight_bar():
    steps = (True, False, True, True)
    assert adam_run(TS.DEFAULT_HYPER, updates=steps)[2] <= 1.0
    for hyper in TS.HYPER_SETS:
        assert adam_run(hyper, updates=steps, count_every_launch=True)[2] > 1e3, hyper


# ------------------------------------------------------------------------------------------------- running statistics
def deep_layer(seed=3):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((2, 128, 12)) * rng.uniform(0.1, 4.0, (1, 128, 1)) + rng.standard_normal((1, 128, 1))).astype(np.float32)
    return z, rng.standard_normal(128).astype(np.float32), rng.uniform(0.5, 2.0, 128).astype(np.float32)


@pytest.mark.parametrize("momentum", [0.1, 0.3, 1.0])
def test_running_statistics_emulation_and_mutations(momentum):
    z, rm, rv = deep_layer()  # N = 24: the unbiased factor is 24 / 23
    want_m, want_v, bar_m, bar_v = TS.running_stats(z, rm, rv, momentum)
    got_m, got_v = TS.running_emulated(z, rm, rv, momentum)
    assert TS.ratio(got_m, want_m, bar_m) <= 1.0 and TS.ratio(got_v, want_v, bar_v) <= 1.0
    if momentum == 1.0:  # whatever came before
        other_m, other_v = TS.running_emulated(z, rm + 7.0, 3.0 * rv, momentum)
        assert np.array_equal(other_m, got_m) and np.array_equal(other_v, got_v)
    _, biased = TS.running_emulated(z, rm, rv, momentum, "biased_variance")
    assert TS.ratio(biased, want_v, bar_v) > 100.0
    if momentum != 0.1:
        dm, dv = TS.running_emulated(z, rm, rv, momentum, "default_momentum")
        assert TS.ratio(dm, want_m, bar_m) > 100.0 and TS.ratio(dv, want_v, bar_v) > 100.0


# --------------------------------------------------------------------------------------------------------------- head
def head_case(labels, bf16, B=3, T=3001, seed=5):
    """Post-ReLU activations and an output layer whose logit gaps pass the expf underflow on most samples."""
    rng = np.random.default_rng(seed)
    a = np.maximum(rng.standard_normal((B, 8, T)), 0.0).astype(np.float32) * 2.0
    if bf16:
        a = TS.round_bf16(a)
    w = (rng.standard_normal((3, 8)) * 60.0).astype(np.float32)
    b = (rng.standard_normal(3) * 20.0).astype(np.float32)
    z = np.einsum("ck,bkt->bct", w.astype(np.float64), a.astype(np.float64)) + b[None, :, None]
    t = np.arange(T)
    y = np.zeros((B, 3, T))
    for i in range(B):
        y[i, 0] = np.exp(-((t - 400.0 - 300 * i) ** 2) / 800.0)
        y[i, 1] = np.exp(-((t - 1500.0 - 200 * i) ** 2) / 800.0)
    y[:, 2] = np.clip(1.0 - y[:, 0] - y[:, 1], 0.0, 1.0)
    if labels == "onehot":  # on the class the logits rule out
        y = np.eye(3)[z.argmin(1)].transpose(0, 2, 1)
    if labels == "zero_window":
        y[1] = 0.0
    return a, w, b, y.astype(np.float32)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("eps", [1e-3, 1e-5, 1e-7])
@pytest.mark.parametrize("labels", ["onehot", "zero_window", "gaussian"])
def test_head_emulation_stays_inside_the_bars_at_saturated_logits(labels, eps, bf16):
    a, w, b, y = head_case(labels, bf16)
    ref = TS.head(a, w, b, y, eps, bf16=bf16)
    gap = ref.z.max(1) - ref.z.min(1)
    assert (gap > 104.0).mean() > 0.5 and ref.eps_share > 0.5, (float((gap > 104.0).mean()), ref.eps_share)
    p, ga, loss, gb, gw = TS.head_emulated(a, w, b, y, eps, bf16=bf16)
    assert ((p == 0.0).any(1)).mean() > 0.5
    assert np.isfinite(loss) and all(np.all(np.isfinite(v)) for v in (p, ga, gb, gw))
    r = {"p": TS.ratio(p, ref.p, ref.bar_p), "loss": abs(loss - ref.loss) / ref.bar_loss, "ga": TS.ratio(ga, ref.ga, ref.bar_ga),
         "gb": TS.ratio(gb, ref.gb, ref.bar_gb), "gw": TS.ratio(gw, ref.gw, ref.bar_gw)}
    print("\n" + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    if labels == "zero_window":
        assert ref.window_loss[1] == 0.0 and not ref.ga[1].any() and not ga[1].any()


@pytest.mark.parametrize("mutation,trips", [
    ("default_loss_eps", ("loss", "ga", "gb", "gw")),
    ("eps_outside_log", ("loss",)),
    ("scale_one_over_B", ("loss", "ga", "gb", "gw")),
    ("unshifted_softmax", ("p",)),
])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_head_mutations_exceed_the_bars(mutation, trips, bf16):
    a, w, b, y = head_case("gaussian", bf16)
    eps = 1e-3
    ref = TS.head(a, w, b, y, eps, bf16=bf16)
    p, ga, loss, gb, gw = TS.head_emulated(a, w, b, y, eps, bf16=bf16, mutation=mutation)
    with np.errstate(all="ignore"):
        r = {"p": TS.ratio(p, ref.p, ref.bar_p), "loss": abs(loss - ref.loss) / ref.bar_loss if np.isfinite(loss) else np.inf,
             "ga": TS.ratio(ga, ref.ga, ref.bar_ga), "gb": TS.ratio(gb, ref.gb, ref.bar_gb), "gw": TS.ratio(gw, ref.gw, ref.bar_gw)}
    print("\n" + mutation + " " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for k in trips:
        assert r[k] > 10.0, (k, r)
