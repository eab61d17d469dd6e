"""Helpers of the EQTransformer batch and loss tests (not a test module): a numpy float64 restatement of block 1's batch
(window, P / S labels without a noise row, SeisBench's detection box written from the named constants of
``volpick_amd.generate``), the adversarial onsets both test files use, the weighted BCE in ``np.longdouble`` with its
a-priori error bars, and the input kinds of the loss tests."""
import numpy as np

from volpick_amd import generate as G

U = 2.0 ** -53  # unit roundoff of float64


# ------------------------------------------------------------------------------------------------------------ the batch
def detection_row(onsets, T, fixed_window=None):
    """SeisBench's ``DetectionLabeller(p_phases, s_phases=s_phases)``, ndim == 2, on the four window-relative onsets
    P, P, S, S (float64, NaN = none): the (T,) row of 0 and 1.  ``fixed_window`` (samples): ``DetectionLabeller(p_phases,
    fixed_window=...)``.  Python floats: the product rounds before the sum."""
    assert G.DETECTION_FACTOR == 1.4 and G.DETECTION_ONSET == "earliest" and G.DETECTION_INDEX is np.trunc
    assert G.DETECTION_NEEDS == "P and S" and G.DETECTION_ORDER == "s >= p"
    y = np.zeros(T)
    factor = G.DETECTION_FACTOR
    p_arrivals = [float(o) for o in onsets[:2] if np.isfinite(o)]
    if fixed_window is not None:
        s_arrivals = [p + float(np.float32(fixed_window)) for p in p_arrivals]  # (the C argument is a float)
        factor = 0
    else:
        s_arrivals = [float(o) for o in onsets[2:] if np.isfinite(o)]
    if len(p_arrivals) != 0 and len(s_arrivals) != 0:
        p, s = min(p_arrivals), min(s_arrivals)
        if s >= p:
            p0 = max(int(G.DETECTION_INDEX(p)), 0)
            p1 = max(int(G.DETECTION_INDEX(s + factor * (s - p))), 0)
            y[p0:p1] = 1
    return y


# (name, window-relative P, P, S, S, fixed_window, the slice [p0, p1) worked out by hand: y[p0:p1] = 1)
NAN = float("nan")
ADVERSARIAL_ONSETS = [
    ("no P", [NAN, NAN, 100.0, NAN], None, (0, 0)),
    ("no S", [100.0, NAN, NAN, NAN], None, (0, 0)),
    ("S before P", [500.0, NAN, 400.0, NAN], None, (0, 0)),
    ("S equal to P", [500.0, NAN, 500.0, NAN], None, (500, 500)),
    ("two P and two S", [700.0, 300.5, 1200.0, 900.25], None, (300, 1739)),   # 900.25 + 1.4 * 599.75 = 1739.9
    ("second column alone", [NAN, 250.0, NAN, 450.0], None, (250, 730)),      # 450 + 1.4 * 200 = 730
    ("P negative, S inside", [-50.5, NAN, 200.0, NAN], None, (0, 550)),       # int(-50.5) = -50 -> 0; 200 + 350.7
    ("p1 beyond T", [5000.0, NAN, 5900.0, NAN], None, (5000, 7160)),
    ("p1 <= p0: all before the window", [-3000.0, NAN, -2000.0, NAN], None, (0, 0)),  # end = -600
    ("p1 <= p0: all behind the window", [7000.0, NAN, 7100.0, NAN], None, (7000, 7240)),
    ("end truncates toward zero", [-10.0, NAN, -4.5, NAN], None, (0, 3)),     # -4.5 + 7.7 = 3.2
    ("half-sample onsets", [100.5, NAN, 300.5, NAN], None, (100, 580)),       # 300.5 + 280 = 580.5
    ("fixed window", [100.5, NAN, NAN, NAN], 1000.0, (100, 1100)),
    ("fixed window ignores S", [100.5, NAN, 50.0, NAN], 250.5, (100, 351)),
    ("fixed window, two P", [400.0, 150.25, NAN, NAN], 100.0, (150, 250)),
    ("fixed window of 0", [400.0, NAN, 900.0, NAN], 0.0, (400, 400)),
    ("fused multiply-add would give 581", [-2304.0, NAN, -1101.5, NAN], None, (0, 582)),
]


def restate(traces, onsets, rows, T, sigma, norm, label_rows, fixed_window=None):
    """The batch the plan rows define, in float64: gather with zero fill, demean, / (max|x| or np.std) + 1e-10; Gaussian
    P and S rows (maximum over a phase's onsets, no noise row, no rescaling) and the detection row, placed by
    ``label_rows`` = the rows of detection, P and S."""
    B = len(rows)
    x = np.zeros((B, 3, T))
    y = np.zeros((B, 3, T))
    t = np.arange(T, dtype=np.float64)
    i_det, i_p, i_s = label_rows
    for b, r in enumerate(rows):
        tr = traces[int(r["trace"])]
        idx = int(r["start"]) + np.arange(T)
        m = (idx >= r["lo"]) & (idx < r["hi"])
        w = np.zeros((3, T))
        w[:, m] = tr[:, idx[m]].astype(np.float64)
        w = w - w.mean(-1, keepdims=True)
        amp = np.abs(w).max(-1, keepdims=True) if norm == "peak" else w.std(-1, keepdims=True)
        x[b] = w / (amp + 1e-10)
        rel = np.asarray(onsets[int(r["trace"])], np.float64) - float(r["start"])
        ph = np.zeros((2, T))
        for j, o in enumerate(rel):
            if np.isfinite(o):
                ph[j // 2] = np.maximum(ph[j // 2], np.exp(-((t - o) ** 2) / (2.0 * sigma ** 2)))
        y[b, i_p], y[b, i_s] = ph
        y[b, i_det] = detection_row(rel, T, fixed_window)
    return x, y


# ------------------------------------------------------------------------------------------------------------- the loss
def bce_truth(p, y, weights):
    """(heads (B, C), windows (B,), batch, S (B, C)) of the weighted BCE in ``np.longdouble``, rounded to float64 at the
    end; S[b][c] = sum_t |term|, what the bars scale with."""
    p, y = np.asarray(p, np.longdouble), np.asarray(y, np.longdouble)
    w = np.asarray(weights, np.longdouble)
    with np.errstate(all="ignore"):
        term = -(y * np.maximum(np.log(p), -100) + (1 - y) * np.maximum(np.log(1 - p), -100))
    heads = term.mean(-1)
    windows = (heads * w).sum(-1)
    return heads.astype(np.float64), windows.astype(np.float64), float(windows.mean()), np.abs(term).sum(-1).astype(np.float64)


def bars(p, y, weights):
    """A-priori bars (head (B, C), window (B,), batch) between a float64 evaluation and the longdouble truth, from the
    roundings alone -- none from a run.  With u = 2^-53, S = sum_t |term| of a row and n = C T:

    * the order of a sum of n float64 terms errs by at most (n - 1) u sum|terms| to first order; two orders (the kernel's
      strided partials and folds, numpy's pairwise sums) differ by twice that: 2 n u S / T in a head.  A head has T terms;
      the bar takes n = C T for it too, so that a route summing a window's C T terms at once is covered;
    * ``1 - p`` rounds where p < 2^-29 carries bits below 2^-53: an absolute error of u / 2 in an argument near 1, so of at
      most u in its logarithm and, times (1 - y) <= 1, in the term: u per term, u in the mean over T;
    * a logarithm correct to 2 ulp moves its product by 4 u |product|; the product and the sum of the two products round
      once each (u |term| each; both products have the sign of the term for y in [0, 1], so |product| <= |term|), the
      division by T once more: 10 u S / T covers them with room.

    head bar   = (2 n + 10) u S / T + u
    window bar = sum_c |w_c| head bar_c + 2 C u sum_c |w_c head_c|     (C products and C - 1 sums)
    batch bar  = mean_b window bar_b + 2 B u mean_b |L_b|              (the sum over the windows, as valloss_f64.batch_bar)"""
    heads, windows, _, S = bce_truth(p, y, weights)
    B, C, T = np.shape(p)
    w = np.abs(np.asarray(weights, np.float64))
    head_bar = (2.0 * C * T + 10.0) * U * S / T + U
    window_bar = (head_bar * w).sum(-1) + 2.0 * C * U * (np.abs(heads) * w).sum(-1)
    batch_bar = float(window_bar.mean() + 2.0 * B * U * np.abs(windows).mean())
    return head_bar, window_bar, batch_bar


def _gauss_rows(B, C, T, rng):
    """Labels as the batch kernel writes them: row 0 a box of ones, the others a Gaussian of width 20."""
    t = np.arange(T, dtype=np.float64)
    y = np.zeros((B, C, T))
    for c in range(C):
        o = rng.uniform(-0.1 * T, 1.1 * T, B)
        if c == 0:
            y[:, c] = (t[None] >= np.floor(o)[:, None]) & (t[None] < np.floor(o + rng.uniform(0, T, B))[:, None])
        else:
            y[:, c] = np.exp(-((t[None] - o[:, None]) ** 2) / (2.0 * 20.0 ** 2))
    return y.astype(np.float32)


def make_inputs(kind, shape, seed=0):
    """(p, y) fp32 of ``shape`` = (B, C, T) for the input kinds of the loss tests."""
    B, C, T = shape
    rng = np.random.default_rng(seed)
    p = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 3.0, shape)))).astype(np.float32)  # what a sigmoid head gives
    y = _gauss_rows(B, C, T, rng)
    if kind == "sigmoid":  # Gaussian and box labels
        assert (p > 0).all() and (p < 1).all()
    elif kind == "clamped":  # p == 0 under y == 1 and p == 1 under y == 0: terms of exactly 100
        lo, n = T // 5, max(1, T // 4)
        p[:, :, lo:lo + n], y[:, :, lo:lo + n] = 0.0, 1.0
        p[:, :, lo + n:lo + 2 * n], y[:, :, lo + n:lo + 2 * n] = 1.0, 0.0
    elif kind == "p_denormal":  # log p from -103.3 (clamped) to -87.3
        p[:] = (rng.integers(1, 1 << 22, shape) * np.float64(2.0 ** -149)).astype(np.float32)
        assert (p > 0).all() and (p < np.finfo(np.float32).tiny).all()
    elif kind == "y_zero":
        y[:] = 0.0
    elif kind == "y_fractional":
        y[:] = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    else:
        raise ValueError(kind)
    return p, y


INPUT_KINDS = ("sigmoid", "clamped", "p_denormal", "y_zero", "y_fractional")
WEIGHTS = (0.05, 0.40, 0.55)


def weights_for(C):
    """The reference's three weights, repeated or cut to C rows."""
    return np.resize(np.array(WEIGHTS), C)
