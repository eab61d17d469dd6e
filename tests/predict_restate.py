"""The five reductions of the reference's ``predict_step`` (volpick/model/models.py:454-480, :881-906) restated in numpy,
with the rules the library pins (include/volpick_hip.h, vp_predict_windows):

* argmax: the lowest index among equal maxima; a NaN is above every number and the first NaN wins;
* max: the value at that index, so a NaN in a row makes the row's maximum NaN;
* PhaseNet's detection score: every ``1 - noise[t]`` is a float32 subtraction, then the maximum;
* ``score_p_or_s``: the float32 quotient of the two maxima, ``x / 0 = inf`` and ``0 / 0 = NaN``.

Also the border cases and adversarial rows the CPU and GPU tests share."""
import numpy as np

ONE_MINUS_NOISE, DET_ROW = 0, 1  # VP_DET_*
RECORD = np.dtype([("det", np.float32), ("p_max", np.float32), ("s_max", np.float32), ("p_arg", np.int32), ("s_arg", np.int32)])


def argmax(row):
    row = np.asarray(row, np.float32)
    if row.size == 0:
        raise ValueError("argmax of an empty border")  # torch raises as well
    nan = np.isnan(row)
    return int(np.flatnonzero(nan)[0]) if nan.any() else int(np.flatnonzero(row == row.max())[0])


def records(prob, det_row, p_row, s_row, det_mode, lo=None, hi=None):
    """prob: (B, n_rows, T) float32 -> a RECORD array of B."""
    prob = np.asarray(prob, np.float32)
    B, _, T = prob.shape
    out = np.zeros(B, RECORD)
    for b in range(B):
        a, e = (0, T) if lo is None else (int(lo[b]), int(hi[b]))
        det, p, s = prob[b, det_row, a:e], prob[b, p_row, a:e], prob[b, s_row, a:e]
        if det_mode == ONE_MINUS_NOISE:
            det = np.float32(1) - det
        out["det"][b] = det[argmax(det)]
        out["p_arg"][b], out["s_arg"][b] = argmax(p), argmax(s)
        out["p_max"][b], out["s_max"][b] = p[out["p_arg"][b]], s[out["s_arg"][b]]
    return out


def predict_step(rec):
    """Records -> (score_detection, score_p_or_s, p_sample, s_sample) as float32, float32, int64, int64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = rec["p_max"].astype(np.float32) / rec["s_max"].astype(np.float32)
    return rec["det"].astype(np.float32), q, rec["p_arg"].astype(np.int64), rec["s_arg"].astype(np.int64)


def same_floats(a, b):
    """Bitwise equal, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_records(a, b):
    return (same_floats(a["det"], b["det"]) and same_floats(a["p_max"], b["p_max"]) and same_floats(a["s_max"], b["s_max"])
            and np.array_equal(a["p_arg"], b["p_arg"]) and np.array_equal(a["s_arg"], b["s_arg"]))


def border_cases(T):
    """(lo, hi) pairs: the smallest that can break a kernel that reads a scalar head, float4 groups and a scalar tail with
    256 threads in 4 waves."""
    cases = [(0, T), (0, 1), (T - 1, T)]                                # whole window, width 1 at either end
    cases += [(5, 5 + w) for w in (1, 63, 64, 65, 257)]                 # lo odd
    cases += [(100 + k, 100 + k + w) for k in (1, 2, 3) for w in (64, 257)]  # lo % 4 in {1, 2, 3}
    cases += [(T - w, T) for w in (63, 65, 257)]                        # hi = T
    cases += [(8, 8 + 4 * 256 * 2 + 3), (1, T)]                         # every thread two groups; all but the first sample
    return [(lo, hi) for lo, hi in cases if 0 <= lo < hi <= T]


ROW_KINDS = ["max_first", "max_last", "outside_larger", "all_equal", "two_waves", "one_nan", "two_nans", "plus_inf", "s_zero",
             "both_zero", "noise_min_first", "noise_min_last", "noise_outside_smaller", "noise_nan"]


def adversarial_window(kind, T, lo, hi, rng, noise_row, p_row, s_row):
    """One (3, T) float32 window of probabilities in (0.05, 0.6) with `kind` planted inside or around [lo, hi)."""
    w = rng.uniform(0.05, 0.6, (3, T)).astype(np.float32)
    n = hi - lo
    far = lo + min(n - 1, 200)  # a sample of another wave than lo's where the border is wide enough
    if kind == "max_first":
        w[p_row, lo] = w[s_row, lo] = 0.9
    elif kind == "max_last":
        w[p_row, hi - 1] = w[s_row, hi - 1] = 0.9
    elif kind == "outside_larger":
        w[p_row, lo] = 0.7
        if lo > 0:
            w[:, lo - 1] = (0.99, 0.99, 0.99)
            w[noise_row, lo - 1] = 0.0
        if hi < T:
            w[:, hi] = (0.99, 0.99, 0.99)
            w[noise_row, hi] = 0.0
    elif kind == "all_equal":
        w[p_row] = 0.25
        w[s_row] = 0.5
        w[noise_row] = 0.125
    elif kind == "two_waves":
        w[p_row, [lo + n // 3, far]] = 0.9
        w[s_row, [lo, hi - 1]] = 0.8
    elif kind == "one_nan":
        w[p_row, lo + n // 2] = np.nan
    elif kind == "two_nans":
        w[s_row, [lo + n // 3, hi - 1]] = np.nan
        w[p_row, [lo, far]] = np.nan
    elif kind == "plus_inf":
        w[p_row, lo + n // 2] = np.inf
        w[s_row, [lo + n // 4, hi - 1]] = np.inf
    elif kind == "s_zero":
        w[s_row] = 0.0
    elif kind == "both_zero":
        w[p_row] = w[s_row] = 0.0
    elif kind == "noise_min_first":
        w[noise_row, lo] = 0.01
    elif kind == "noise_min_last":
        w[noise_row, hi - 1] = 0.01
    elif kind == "noise_outside_smaller":
        if lo > 0:
            w[noise_row, lo - 1] = 0.0
        if hi < T:
            w[noise_row, hi] = 0.0
        w[noise_row, [lo + n // 3, far]] = 0.02
    elif kind == "noise_nan":
        w[noise_row, hi - 1] = np.nan
    else:
        raise ValueError(kind)
    return w


def adversarial_batch(T, B, seed, noise_row=2, p_row=0, s_row=1):
    """(prob (B, 3, T), lo, hi): window b gets border case b and row kind b, both cycling, so that 37 windows cover every
    kind and every border and every kind meets several borders."""
    rng = np.random.default_rng(seed)
    cases = border_cases(T)
    lo = np.array([cases[(b + seed) % len(cases)][0] for b in range(B)], np.int32)
    hi = np.array([cases[(b + seed) % len(cases)][1] for b in range(B)], np.int32)
    prob = np.stack([adversarial_window(ROW_KINDS[b % len(ROW_KINDS)], T, lo[b], hi[b], rng, noise_row, p_row, s_row)
                     for b in range(B)])
    return prob, lo, hi
