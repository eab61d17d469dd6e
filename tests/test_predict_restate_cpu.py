"""CPU: the numpy restatement of predict_step's reductions (tests/predict_restate.py) against the same reductions written
with torch ops on the CPU, as the reference writes them (volpick/model/models.py:454-480, :881-906)."""
import numpy as np
import pytest
import torch

from tests import predict_restate as R


def torch_predict_step(prob, det_row, p_row, s_row, det_mode, lo, hi):
    pred = torch.from_numpy(prob)
    n = pred.shape[0]
    det, q = torch.zeros(n), torch.zeros(n)
    p_sample, s_sample = torch.zeros(n, dtype=int), torch.zeros(n, dtype=int)
    for i in range(n):
        local = pred[i, :, int(lo[i]):int(hi[i])]
        det[i] = torch.max(1 - local[det_row]) if det_mode == R.ONE_MINUS_NOISE else torch.max(local[det_row])
        q[i] = torch.max(local[p_row]) / torch.max(local[s_row])
        p_sample[i] = torch.argmax(local[p_row])
        s_sample[i] = torch.argmax(local[s_row])
    return det.numpy(), q.numpy(), p_sample.numpy(), s_sample.numpy()


def check(prob, rows, mode, lo, hi):
    got = R.predict_step(R.records(prob, *rows, mode, lo, hi))
    want = torch_predict_step(prob, *rows, mode, lo, hi)
    assert [g.dtype for g in got] == [np.float32, np.float32, np.int64, np.int64]
    assert R.same_floats(got[0], want[0]) and R.same_floats(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    return got


@pytest.mark.parametrize("T", [3001, 6000])
@pytest.mark.parametrize("mode,rows", [(R.ONE_MINUS_NOISE, (2, 0, 1)), (R.ONE_MINUS_NOISE, (0, 1, 2)), (R.DET_ROW, (0, 1, 2))])
def test_random_rows(T, mode, rows):
    rng = np.random.default_rng(T + mode)
    B = 24
    prob = rng.random((B, 3, T), dtype=np.float32)
    lo = rng.integers(0, T - 1, B)
    hi = np.array([rng.integers(a + 1, T + 1) for a in lo])
    check(prob, rows, mode, lo, hi)
    check(prob, rows, mode, np.zeros(B, int), np.full(B, T))
    assert R.same_records(R.records(prob, *rows, mode), R.records(prob, *rows, mode, np.zeros(B, int), np.full(B, T)))


@pytest.mark.parametrize("T", [3001, 6000])
@pytest.mark.parametrize("seed", range(4))
def test_adversarial_rows(T, seed):
    mode = R.ONE_MINUS_NOISE if T == 3001 else R.DET_ROW
    rows = (2, 0, 1) if T == 3001 else (0, 1, 2)  # PhaseNet "PSN": noise, P, S; EQTransformer: detection, P, S
    prob, lo, hi = R.adversarial_batch(T, 37, seed, noise_row=rows[0], p_row=rows[1], s_row=rows[2])
    det, q, p, s = check(prob, rows, mode, lo, hi)
    kinds = [R.ROW_KINDS[b % len(R.ROW_KINDS)] for b in range(37)]
    for b, kind in enumerate(kinds):
        n = hi[b] - lo[b]
        if kind == "max_first":
            assert p[b] == s[b] == 0
        elif kind == "max_last":
            assert p[b] == s[b] == n - 1
        elif kind == "all_equal":
            assert p[b] == s[b] == 0 and q[b] == np.float32(0.5)
        elif kind == "two_waves":
            assert p[b] == min(n // 3, n - 1, 200) and s[b] == 0
        elif kind == "one_nan":
            assert p[b] == n // 2 and np.isnan(q[b])
        elif kind == "two_nans":
            assert p[b] == 0 and s[b] == n // 3 and np.isnan(q[b])
        elif kind == "s_zero":
            assert q[b] == np.inf
        elif kind == "both_zero":
            assert np.isnan(q[b]) and p[b] == s[b] == 0
        elif kind == "plus_inf":
            assert p[b] == n // 2 and s[b] == n // 4
        elif kind == "noise_nan" and mode == R.ONE_MINUS_NOISE:
            assert np.isnan(det[b])
        elif kind == "noise_min_first" and mode == R.ONE_MINUS_NOISE:
            assert det[b] == np.float32(1) - np.float32(0.01)
        elif kind == "outside_larger":
            assert det[b] < 0.96 and q[b] < 20
    assert {(int(a), int(e)) for a, e in zip(lo, hi)} == set(R.border_cases(T))  # 37 windows meet every border case


def test_an_empty_border_raises():
    with pytest.raises(ValueError):
        R.records(np.zeros((1, 3, 16), np.float32), 0, 1, 2, R.DET_ROW, [4], [4])
