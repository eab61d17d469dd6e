"""What surrounds the conv / BatchNorm / weight-gradient launches of the PhaseNet training step, at its edges: the optimiser
state over several updates, non-default hyper-parameters, the BatchNorm running statistics, the loss head at a saturated
softmax, vp_train_write_weights, the EMA and vp_train_set_hyper's argument checks.  Every update is compared in float64
with the values that update itself read (tests/train_state_f64.py: restatements and a-priori bars), so the bars are rounding
bars; tests/test_train_state_cpu.py shows what each of them catches.  The module prints the worst got / bar per assertion
(profiles/train_state_gpu_tests.txt is that output)."""
import functools

import numpy as np
import pytest

from tests import train_state_f64 as TS
from tests.test_gpu_train import make_batch
from volpick_amd import PhaseNet, _lib
from volpick_amd.train import PhaseNetTrainer

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
# (update, lr, B): B = 2, 3, 6 are the head grids; at B = 2 the deepest layers normalise over N = 24 values
STEPS = ((True, 1e-3, 6), (False, 1e-3, 3), (True, 5e-4, 2), (True, 0.0, 6), (True, 2e-3, 6))
REPORT = {}


def note(name, r):
    REPORT[name] = max(REPORT.get(name, 0.0), float(r))
    return r


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst got / bar per assertion (figure: worst |got - ref| in u of the magnitude, see tests/train_state_f64.py)")
    for k in sorted(REPORT):
        print(f"  {k:44s} {REPORT[k]:.4g}")


@functools.lru_cache(maxsize=None)
def batch(B):
    x, y = make_batch(B, 40 + B)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.fixture(scope="module")
def shipped():
    w = np.array(PhaseNet.from_pretrained("volpick")._weights, dtype=np.float32)
    w.setflags(write=False)
    return w


def trainer(dtype, hyper=TS.DEFAULT_HYPER):
    b1, b2, eps, mom, leps = hyper
    return PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=8, betas=(b1, b2), eps=eps, bn_momentum=mom,
                           loss_eps=leps, dtype=dtype)


class State:
    """Everything the trainer hands back after a step."""

    def __init__(self, tr, B=None, loss=None):
        self.w, self.g = tr.weights(), tr.gradients()
        self.m, self.v = tr.adam_state()
        self.t = tr.tensors(B) if B else None
        self.p = tr.predictions(B) if B else None
        self.loss = loss


def trainable(w):
    return [k for k in w if "running_" not in k]


def bit_equal(a, b, keys=None):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in (keys if keys is not None else a))


def check_adam(before, after, t, lr, hyper, tag):
    """The update that led from ``before`` to ``after``: every trainable element, none exempt."""
    worst = np.zeros(4)
    for k in trainable(after.w):
        ref = TS.adam_update(before.w[k], after.g[k], before.m[k], before.v[k], t, lr, *hyper[:3])
        r = [TS.ratio(after.m[k], ref.m, ref.bar_m), TS.ratio(after.v[k], ref.v, ref.bar_v),
             TS.ratio(after.w[k], ref.w, ref.bar_w), TS.ratio(after.w[k], ref.w, ref.bar_w_plain)]
        worst = np.maximum(worst, r)
        assert max(r[:3]) <= 1.0, (tag, k, t, r)
    note("adam m", worst[0]), note("adam v", worst[1]), note("adam w", worst[2])
    note("adam w (plain bar, reported only)", worst[3])
    print(f"{tag}: adam t={t} lr={lr:g}  m {worst[0]:.3f} v {worst[1]:.3f} w {worst[2]:.3f} (plain {worst[3]:.3f})")


def check_running(before, after, momentum, tag):
    worst = 0.0
    for bn, layer in TS.BN_LAYERS.items():
        z = after.t[layer + ".z"]
        rm, rv, bar_m, bar_v = TS.running_stats(z, before.w[bn + ".running_mean"], before.w[bn + ".running_var"], momentum)
        r = max(TS.ratio(after.w[bn + ".running_mean"], rm, bar_m), TS.ratio(after.w[bn + ".running_var"], rv, bar_v))
        assert r <= 1.0, (tag, bn, z.shape, r)
        worst = max(worst, r)
    note("running statistics", worst)
    return worst


def check_head(before, after, y, loss_eps, dtype, tag, figures=False):
    """Loss, predictions, up3.same.ga and the out.* gradients of the step that led to ``after`` (the weights it read are
    ``before``'s) against the float64 head on its own stored up3.same.a."""
    bf16 = dtype == "bf16"
    ref = TS.head(after.t["up3.same.a"], before.w["out.weight"].reshape(3, 8), before.w["out.bias"], y, loss_eps, bf16=bf16)
    got = {"p": after.p, "ga": after.t["up3.same.ga"], "gb": after.g["out.bias"], "gw": after.g["out.weight"].reshape(3, 8)}
    assert np.isfinite(after.loss) and all(np.all(np.isfinite(v)) for v in got.values()), tag
    r = {"p": TS.ratio(got["p"], ref.p, ref.bar_p), "loss": abs(after.loss - ref.loss) / ref.bar_loss,
         "ga": TS.ratio(got["ga"], ref.ga, ref.bar_ga), "gb": TS.ratio(got["gb"], ref.gb, ref.bar_gb),
         "gw": TS.ratio(got["gw"], ref.gw, ref.bar_gw)}
    for k, v in r.items():
        note(f"head {k} {dtype}", v)
    if figures:  # shipped weights only: what K_EXP and K_LOG are four times of
        big = ref.p > 0.01  # (below, the rounding of the argument z - max z itself, u |z - max z|, outgrows the function's)
        note("figure expf (u of p, p > 0.01)", (np.abs(got["p"] - ref.p)[big] / (TS.U * ref.p[big])).max())
        note("figure logf (u of sum |y log q| scale)", abs(after.loss - ref.loss) / (TS.U * ref.log_mag))
    print(f"{tag}: head eps={loss_eps:g} " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (tag, r)
    return ref, got


@pytest.mark.parametrize("hyper", TS.HYPER_SETS, ids=["defaults", "b.5_.9_eps1e-3_mom.3", "b.8_.99_eps1e-6_mom1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_five_steps_follow_adam_and_the_running_statistics_in_float64(dtype, hyper):
    tr = trainer(dtype, hyper)
    cur = State(tr)
    assert not any(cur.m[k].any() or cur.v[k].any() for k in cur.m)
    t = 0
    for i, (update, lr, B) in enumerate(STEPS):
        x, y = batch(B)
        tag = f"{dtype} step {i + 1}"
        loss = tr.step(x, y, lr, update=update)
        new = State(tr, B, loss)
        keys = trainable(new.w)
        r = check_running(cur, new, hyper[3], tag)  # every step moves them, an update=False one too
        print(f"{tag}: running statistics B={B} {r:.3f}")
        check_head(cur, new, y, hyper[4], dtype, tag, figures=True)  # the gradients are this batch's
        if update:
            t += 1  # updates, not launches: the update behind the update=False step has t = 2
            check_adam(cur, new, t, lr, hyper, tag)
            assert not bit_equal(cur.m, new.m, keys) and not bit_equal(cur.v, new.v, keys)
            if lr == 0.0:
                assert bit_equal(cur.w, new.w, keys)
        else:
            assert bit_equal(cur.w, new.w, keys) and bit_equal(cur.m, new.m) and bit_equal(cur.v, new.v)
            assert not bit_equal(cur.g, new.g, keys)
            assert not bit_equal(cur.w, new.w, [k for k in new.w if "running_" in k])
        cur = new
    assert t == 4 and tr.global_step == 4
    tr.close()


# ------------------------------------------------------------------------------------------------ head at its edges
_EDGE = {}


@pytest.fixture(scope="module")
def edge_trainers():
    yield _EDGE
    for tr in _EDGE.values():
        tr.close()
    _EDGE.clear()


def edge_labels(kind, y, z):
    y = np.array(y)
    if kind == "onehot":  # hard labels on the class the logits rule out: every term of the loss is -log(0 + eps)
        y = np.ascontiguousarray(np.eye(3, dtype=np.float32)[z.argmin(1)].transpose(0, 2, 1))
    if kind == "zero_window":
        y[1] = 0.0
    return y


@pytest.mark.parametrize("labels", ["onehot", "zero_window", "gaussian"])
@pytest.mark.parametrize("loss_eps", [1e-3, 1e-5, 1e-7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_head_at_a_saturated_softmax(edge_trainers, shipped, dtype, loss_eps, labels):
    B = 3
    key = (dtype, loss_eps)
    if key not in edge_trainers:
        edge_trainers[key] = trainer(dtype, TS.DEFAULT_HYPER[:4] + (loss_eps,))
    tr = edge_trainers[key]
    x, y0 = batch(B)
    tr.step(x, y0, 0.0, update=False)  # up3.same.a does not depend on out.*: batch statistics, no update
    a = tr.tensors(B)["up3.same.a"]
    blob = tr._read(0)
    named, ship = tr._named(blob), tr._named(np.array(shipped))
    w0, b0 = ship["out.weight"].reshape(3, 8).astype(np.float64), ship["out.bias"].astype(np.float64)
    z0 = np.einsum("ck,bkt->bct", w0, a.astype(np.float64)) + b0[None, :, None]
    scale = 110.0 / np.percentile(z0.max(1) - z0.min(1), 20.0)  # four samples in five pass the expf underflow
    named["out.weight"][...] = (scale * w0).reshape(named["out.weight"].shape)
    named["out.bias"][...] = scale * b0
    tr.write_weights(blob)
    before = State(tr)
    assert np.array_equal(before.w["out.bias"], (scale * b0).astype(np.float32))
    z = np.einsum("ck,bkt->bct", before.w["out.weight"].reshape(3, 8).astype(np.float64), a.astype(np.float64)) \
        + before.w["out.bias"].astype(np.float64)[None, :, None]
    y = edge_labels(labels, y0, z)
    loss = tr.step(x, y, 0.0, update=False)
    after = State(tr, B, loss)
    assert np.array_equal(after.t["up3.same.a"], a)
    tag = f"{dtype} {labels}"
    ref, got = check_head(before, after, y, loss_eps, dtype, tag)
    gap = ref.z.max(1) - ref.z.min(1)
    assert (gap > 104.0).mean() > 0.5, float((gap > 104.0).mean())       # on the stored a: the softmax is saturated ...
    assert (got["p"] == 0.0).any(1).mean() > 0.5                          # ... p is exactly 0 for some class on most samples ...
    assert ref.eps_share > 0.5, ref.eps_share                             # ... and eps decides most of the loss
    print(f"{tag}: gaps > 104 on {100 * (gap > 104.0).mean():.0f} %, eps-dominated share of the loss {ref.eps_share:.3f}, "
          f"loss {loss:.4f}")
    if labels == "zero_window":
        assert ref.window_loss[1] == 0.0 and not got["ga"][1].any()
        assert got["ga"][0].any() and got["ga"][2].any()


# ------------------------------------------------------------------------------------------- vp_train_write_weights
@pytest.mark.parametrize("dtype", DTYPES)
def test_write_weights_replaces_the_blob_and_nothing_else(shipped, dtype):
    hyper = TS.HYPER_SETS[1]
    tr = trainer(dtype, hyper)
    x6, y6 = batch(6)
    x3, y3 = batch(3)
    tr.step(x6, y6, 1e-3)
    tr.step(x6, y6, 1e-3)
    moved = State(tr)
    assert not np.array_equal(tr._read(0), shipped)
    tr.write_weights(shipped)
    written = State(tr)
    assert np.array_equal(tr._read(0), shipped)
    assert bit_equal(moved.m, written.m) and bit_equal(moved.v, written.v)
    loss = tr.step(x3, y3, 1e-3, update=False)
    ours = State(tr, 3, loss)
    fresh_tr = trainer(dtype, hyper)
    fresh = State(fresh_tr, 3, fresh_tr.step(x3, y3, 1e-3, update=False))
    fresh_tr.close()
    assert ours.loss == fresh.loss and np.array_equal(ours.p, fresh.p)
    assert bit_equal(ours.g, fresh.g) and bit_equal(ours.t, fresh.t)
    assert bit_equal(ours.w, fresh.w)  # the running statistics moved from the shipped ones, the same way
    assert not np.array_equal(ours.w["in_bn.running_mean"], written.w["in_bn.running_mean"])
    assert bit_equal(moved.m, ours.m) and bit_equal(moved.v, ours.v)
    # the next update goes on from the old moments as update 3
    new = State(tr, 6, tr.step(x6, y6, 1e-3))
    check_adam(ours, new, 3, 1e-3, hyper, f"{dtype} after write_weights")
    assert tr.global_step == 3
    with pytest.raises(ValueError):
        tr.write_weights(shipped[:-1])
    tr.close()


# ---------------------------------------------------------------------------------------------------------------- EMA
@pytest.mark.parametrize("dtype", DTYPES)
def test_ema_from_the_current_weights_through_updates_and_plain_steps(dtype):
    tr = trainer(dtype)
    x, y = batch(6)
    x3, y3 = batch(3)
    tr.step(x, y, 1e-3)
    tr.step(x, y, 1e-3)
    tr.enable_ema(0.9)
    ema = tr.ema_weights()
    assert bit_equal(ema, tr.weights())  # enabled late: it starts at the current weights, not at the initial ones
    running = [k for k in ema if "running_" in k]
    for i in range(2):
        tr.step(x, y, 1e-3)
        w, new = tr.weights(), tr.ema_weights()
        worst = 0.0
        for k in trainable(w):
            want, bar = TS.ema_update(ema[k], w[k], 0.9)
            worst = max(worst, TS.ratio(new[k], want, bar))
            assert worst <= 1.0, (k, worst)
        note("ema", worst)
        print(f"{dtype}: ema update {i + 1} {worst:.3f}")
        assert bit_equal(new, w, running)  # buffers are not averaged: their slots hold the current statistics
        assert not np.array_equal(new["inc.weight"], w["inc.weight"])
        ema = new
    tr.step(x3, y3, 1e-3, update=False)  # no Adam launch: every EMA slot stays, though the statistics have moved
    assert bit_equal(tr.ema_weights(), ema)
    assert not bit_equal(tr.weights(), ema, running)
    tr.enable_ema(0.0)
    tr.step(x, y, 1e-3)
    assert bit_equal(tr.ema_weights(), tr.weights())
    tr.close()


# ---------------------------------------------------------------------------------------------------- argument errors
NAN, INF = float("nan"), float("inf")
VP_ERR_INVALID = -1  # include/volpick_hip.h
GOOD = TS.HYPER_SETS[1]
BAD_HYPER = [
    (1.0, 0.9, 1e-3, 0.3, 1e-3), (-0.1, 0.9, 1e-3, 0.3, 1e-3), (NAN, 0.9, 1e-3, 0.3, 1e-3), (1.5, 0.9, 1e-3, 0.3, 1e-3),
    (0.5, 1.0, 1e-3, 0.3, 1e-3), (0.5, -1e-3, 1e-3, 0.3, 1e-3), (0.5, NAN, 1e-3, 0.3, 1e-3),
    (0.5, 0.9, 0.0, 0.3, 1e-3), (0.5, 0.9, -1e-8, 0.3, 1e-3), (0.5, 0.9, INF, 0.3, 1e-3), (0.5, 0.9, NAN, 0.3, 1e-3),
    (0.5, 0.9, 1e-3, 0.0, 1e-3), (0.5, 0.9, 1e-3, -0.1, 1e-3), (0.5, 0.9, 1e-3, 1.5, 1e-3), (0.5, 0.9, 1e-3, NAN, 1e-3),
    (0.5, 0.9, 1e-3, 0.3, 0.0), (0.5, 0.9, 1e-3, 0.3, -1e-5), (0.5, 0.9, 1e-3, 0.3, INF), (0.5, 0.9, 1e-3, 0.3, NAN),
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_set_hyper_refuses_bad_values_and_keeps_the_previous_ones(dtype, monkeypatch):
    tr = trainer(dtype, GOOD)
    lib = tr._lib
    for bad in BAD_HYPER:
        assert lib.vp_train_set_hyper(tr._h, *bad) == VP_ERR_INVALID, bad
        assert "vp_train_set_hyper" in _lib.last_error()
    before = State(tr)
    x, y = batch(2)
    after = State(tr, 2, tr.step(x, y, 1e-3))  # the refused calls changed nothing: this update runs on GOOD
    check_adam(before, after, 1, 1e-3, GOOD, f"{dtype} after refused set_hyper")
    check_running(before, after, GOOD[3], dtype)
    check_head(before, after, y, GOOD[4], dtype, f"{dtype} after refused set_hyper")
    assert all(np.all(np.isfinite(v)) for v in after.w.values())
    assert lib.vp_train_set_hyper(tr._h, 0.0, 0.0, 1e-30, 1.0, 1e-30) == 0  # the closed ends of the ranges are inside
    tr.close()
    # the constructor raises instead of handing out a trainer whose first update divides by zero, and frees the handle
    destroyed = []
    real = lib.vp_train_destroy
    monkeypatch.setattr(lib, "vp_train_destroy", lambda h: destroyed.append(1) or real(h))
    for kw in ({"betas": (1.0, 0.999)}, {"eps": 0.0}, {"bn_momentum": 0.0}, {"loss_eps": NAN}):
        n = len(destroyed)
        with pytest.raises(_lib.VolpickHipError, match="vp_train_set_hyper"):
            PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=2, dtype=dtype, **kw)
        assert len(destroyed) == n + 1, kw
