"""GPU: the optimiser state both trainers hold (volpick_amd/csrc/train_optim.hip) through vp_train_read / _write_weights and
vp_eqt_dec_train_read / _write_weights: every selector, the refusals with their texts, and that a written blob leaves the
moments and the update count alone.  A PhaseNet trainer at max_batch = 2 and a decoder trainer at max_batch = 1, one update
each at that batch; the update behind write_weights is compared with the float64 Adam of tests/train_state_f64.py at that
module's bars."""
import numpy as np
import pytest

from tests import train_state_f64 as TS
from tests.test_gpu_eqt_dec_train import make_batch as eqt_batch
from tests.test_gpu_train import make_batch as phasenet_batch
from volpick_amd import EQTransformer, PhaseNet, _lib
from volpick_amd.train import EQT_LOSS_WEIGHTS, EQTransformerDecoderTrainer, PhaseNetTrainer

pytestmark = pytest.mark.gpu

VP_ERR_INVALID = -1  # include/volpick_hip.h
HYPER = TS.DEFAULT_HYPER[:3]
LR = 1e-3


def phasenet():
    tr = PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=2)
    x, y = phasenet_batch(2, 71)
    return tr, (lambda: tr.step(x, y, LR)), "vp_train", "vp_train_write_weights: bad size"


def decoders():
    tr = EQTransformerDecoderTrainer(EQTransformer.from_pretrained("volpick"), max_batch=1)
    x, y = eqt_batch(1, 72)
    n = tr.n_params
    return tr, (lambda: tr.step(x, y, LR, EQT_LOSS_WEIGHTS)), "vp_eqt_dec_train", f"vp_eqt_dec_train_write_weights: expected {n} floats, got "


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("make", [phasenet, decoders])
def test_selectors_sizes_and_write_weights(make):
    tr, step, prefix, bad_write = make()
    lib, n = tr._lib, tr.n_params
    read, write = getattr(lib, prefix + "_read"), getattr(lib, prefix + "_write_weights")
    has_ema = make is phasenet
    w0 = tr._read(0)
    step()

    # ---- selectors 0 .. 3
    w, g, m, v = (tr._read(k) for k in range(4))
    assert all(a.shape == (n,) and a.dtype == np.float32 for a in (w, g, m, v))
    assert m.any() and v.any() and g.any() and (v >= 0).all()
    got = (w, g, m, v)
    assert not any(np.array_equal(got[i], got[j]) for i in range(4) for j in range(i))
    assert not np.array_equal(w, w0)
    named = {k: tr._named(a) for k, a in zip("wgmv", got)}
    train = [k for k in named["w"] if "running_" not in k]
    for k in train:  # the first update from zero moments: m = (1 - b1) g, v = (1 - b2) g^2, at the float64 bars
        ref = TS.adam_update(tr._named(w0)[k], named["g"][k], np.zeros_like(named["g"][k]), np.zeros_like(named["g"][k]), 1, LR, *HYPER)
        assert max(TS.ratio(named["m"][k], ref.m, ref.bar_m), TS.ratio(named["v"][k], ref.v, ref.bar_v),
                   TS.ratio(named["w"][k], ref.w, ref.bar_w)) <= 1.0, k

    # ---- the selectors behind them
    out = np.full(n + 1, 7.0, np.float32)
    for which in (5, -1) + (() if has_ema else (4,)):
        assert read(tr._h, which, _lib.ptr(out), n) == VP_ERR_INVALID, which
        assert f"{prefix}_read: bad size or selector" in _lib.last_error(), which
    if has_ema:
        assert read(tr._h, 4, _lib.ptr(out), n) == VP_ERR_INVALID
        assert "vp_train_read: EMA is off (vp_train_set_ema)" in _lib.last_error()
        tr.enable_ema(0.9)
        assert same_bits(tr._read(4), tr._read(0))

    # ---- sizes off by one: refused by read and by write_weights, nothing copied either way
    for wrong in (n - 1, n + 1):
        assert read(tr._h, 0, _lib.ptr(out), wrong) == VP_ERR_INVALID
        assert f"{prefix}_read: bad size or selector" in _lib.last_error()
        assert write(tr._h, _lib.ptr(out), wrong) == VP_ERR_INVALID
        err = _lib.last_error()
        assert bad_write in err and (has_ema or err.endswith(f"got {wrong}")), err
    assert (out == 7.0).all() and same_bits(tr._read(0), w)

    # ---- write_weights: the blob alone; the next update is update 2 on the old moments
    tr.write_weights(w0)
    assert same_bits(tr._read(0), w0) and same_bits(tr._read(2), m) and same_bits(tr._read(3), v)
    step()
    w2, g2, m2, v2 = (tr._named(tr._read(k)) for k in range(4))
    wrote = tr._named(w0)
    worst, worst_t1 = np.zeros(3), 0.0
    for k in train:
        ref = TS.adam_update(wrote[k], g2[k], named["m"][k], named["v"][k], 2, LR, *HYPER)
        worst = np.maximum(worst, [TS.ratio(m2[k], ref.m, ref.bar_m), TS.ratio(v2[k], ref.v, ref.bar_v), TS.ratio(w2[k], ref.w, ref.bar_w)])
        one = TS.adam_update(wrote[k], g2[k], named["m"][k], named["v"][k], 1, LR, *HYPER)  # (a count that started over)
        worst_t1 = max(worst_t1, TS.ratio(w2[k], one.w, one.bar_w))
    print(f"{prefix}: update 2 behind write_weights, worst error / bar: m {worst[0]:.3g} v {worst[1]:.3g} w {worst[2]:.3g}; "
          f"against update 1's bias correction: w {worst_t1:.3g}")
    assert (worst <= 1.0).all() and worst_t1 > 1.0
    assert tr.global_step == 2
    tr.close()
