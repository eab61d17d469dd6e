"""A float64 numpy restatement of the augmented training window (volpick_amd/generate.py, AugmentedPlanner; the
reference's volpick/model/models.py:345-440 and augmentations.py), written from its description:

* ``decide`` follows the reference's procedure on float64 label arrays -- the first event's end, the truncation, the
  sources' P-label check (np.isclose), np.argmax of the labels, the shifts -- drawing every random choice from an injected
  source, and returns the AUG_ROW record that procedure implies;
* ``execute`` computes the window (x, y) an AUG_ROW record defines;
* ``philox4x32_10`` / ``gauss_noise``: the counter-based generator of the Gaussian-noise slot.
"""
import numpy as np

from volpick_amd import generate as G

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 of counters ctr (4, N) (any integer dtype) under key (k0, k1): (4, N) uint64 words < 2^32."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in ctr]
    k0, k1 = np.uint64(key[0] & MASK), np.uint64(key[1] & MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return c


def gauss_noise(key, T):
    """(3, T) standard normals of the Gaussian-noise slot for a 64-bit key: counter (t, c, 0, 0), Box-Muller (cos)."""
    key = int(key)
    t = np.tile(np.arange(T, dtype=np.uint64), 3)
    c = np.repeat(np.arange(3, dtype=np.uint64), T)
    z = np.zeros_like(t)
    w = philox4x32_10([t, c, z, z], (key & MASK, key >> 32))
    u0 = ((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)
    u1 = ((w[3] << np.uint64(32)) | w[2]) >> np.uint64(11)
    u0 = u0.astype(np.float64) * 2.0 ** -53
    u1 = u1.astype(np.float64) * 2.0 ** -53
    return (np.sqrt(-2.0 * np.log(1.0 - u0)) * np.cos(2.0 * np.pi * u1)).reshape(3, T)


def labels_of(ons, T, sigma):
    """P, S (T,) float64 for window-local onsets (4,) (P, P, S, S; NaN = none)."""
    t = np.arange(T, dtype=np.float64)
    ph = np.zeros((2, T))
    for j, o in enumerate(ons):
        if np.isfinite(o):
            ph[j // 2] = np.maximum(ph[j // 2], np.exp(-((t - o) ** 2) / (2.0 * sigma ** 2)))
    return ph


def window(traces, row, T, norm):
    """Block 1's cut (zero fill), demean and normalisation of a plan row, float64."""
    tr = traces[int(row["trace"])]
    idx = int(row["start"]) + np.arange(T)
    m = (idx >= row["lo"]) & (idx < row["hi"])
    w = np.zeros((3, T))
    w[:, m] = tr[:, idx[m]].astype(np.float64)
    return normalise(w, norm)


def normalise(w, norm):
    w = w - w.mean(-1, keepdims=True)
    amp = np.abs(w).max(-1, keepdims=True) if norm == "peak" else w.std(-1, keepdims=True)
    return w / (amp + 1e-10)


def shift(a, d):
    """a[..., t - d] with zero fill (the reference's shift of a source)."""
    T = a.shape[-1]
    out = np.zeros_like(a)
    if d >= 0:
        if d < T:
            out[..., d:] = a[..., :T - d]
    elif -d < T:
        out[..., :d] = a[..., -d:]
    return out


def execute(rec, traces, onsets, T, sigma, norm, labels):
    """x, y (3, T) float64 of one AUG_ROW record (include/volpick_hip.h, vp_aug_row steps 1-7)."""
    ip, is_, in_ = G.label_rows(labels)
    pr = rec["primary"]
    x0 = window(traces, pr, T, norm)
    pons = onsets[int(pr["trace"])] - float(pr["start"])
    P, S = labels_of(pons, T, sigma)
    x = x0.copy()
    x[:, int(rec["cut"]):] = 0
    renorm = False
    for ev in rec["event"]:
        if ev["kind"] == G.AUG_NONE:
            continue
        if ev["kind"] == G.AUG_BANK:
            s = window(traces, ev["row"], T, norm)
            s[np.all(np.abs(x) <= 1e-8, axis=1)] = 0
            sons = onsets[int(ev["row"]["trace"])] - float(ev["row"]["start"])
        else:
            s, sons = x0.copy(), pons
        s[:, :int(ev["zero_before"])] = 0
        d = int(ev["shift"])
        x = x + float(ev["scale"]) * shift(s, d)
        P2, S2 = shift(labels_of(sons, T, sigma), d)
        P, S = np.maximum(P, P2), np.maximum(S, S2)
        den = np.maximum(1.0, P + S)
        P, S = P / den, S / den
        renorm = True
    for nz in rec["noise"]:
        if nz["kind"] == G.AUG_NONE:
            continue
        s = window(traces, nz["row"], T, norm)
        s[np.all(np.abs(x) <= 1e-8, axis=1)] = 0
        x = x + s * (np.abs(x).max() * float(nz["scale"]))
    if rec["gauss"] > 0:
        x = x + float(rec["gauss"]) * x.max() * gauss_noise(rec["noise_key"], T)
    g0, g1 = int(rec["gap_lo"]), int(rec["gap_hi"])
    x[:, g0:g1] = 0
    P[g0:g1] = 0
    S[g0:g1] = 0
    y = np.zeros((3, T))
    y[ip], y[is_] = P, S
    y[in_] = 1.0 - P - S if renorm else np.clip(1.0 - P - S, 0.0, 1.0)
    return normalise(x, norm), y


class Replay:
    """The random source of one window from AugmentedPlanner.last_draws (window b): the uniforms of generate.U_COLS
    mapped as the planner's docstring says, and the sources' block-1 rows."""

    def __init__(self, draws, b):
        self.u, self.d, self.b = draws["u"][b], draws, b

    def _u(self, name, i=None):
        col = G.U_COLS[name]
        return self.u[col if i is None else col[i]]

    def branch(self, name, probs):
        cum = np.cumsum(np.asarray(probs, float) / np.sum(probs))
        return int(np.searchsorted(cum, self._u(name), side="right"))

    def integer(self, name, i, lo, hi):
        return lo + min(int(np.floor(self._u(name, i) * (hi - lo))), hi - lo - 1)

    def uniform(self, name, i, lo, hi):
        return lo + self._u(name, i) * (hi - lo)

    def source(self, kind, i, subset):
        tr = subset[self.integer(kind + "_source", i, 0, len(subset))]
        assert tr == self.d[kind + "_traces"][self.b, i]
        return tr, self.d[kind + "_rows"][self.b, i]

    def noise_key(self):
        return int(self.d["noise_key"][self.b])


def decide(prim, onsets, event_traces, noise_traces, T, sigma, rnd, event_prob=(0.2, 0.2, 0.6),
           noise_prob=(0.25, 0.25, 0.5), gap_prob=(0.2, 0.8), num=(0.7, 0.3), sep=200, tail=1.4):
    """The AUG_ROW record the reference's procedure implies for the primary row `prim`, with random source `rnd`."""
    rec = np.zeros((), G.AUG_ROW)
    rec["primary"] = prim
    rec["cut"] = T
    ons = onsets[int(prim["trace"])] - float(prim["start"])
    P, S = labels_of(ons, T, sigma)
    if len(event_traces):
        br = rnd.branch("event_branch", event_prob)
        n = 1 + rnd.branch("n_events", num)
        picks = [o for o in ons if np.isfinite(o)]
        sup = br == 0
        go = br < 2 and len(picks) > 0
        if br == 1 and not np.isclose(P.max(), 1, atol=1e-2):
            go = False
        if go:
            if len(picks) >= 2:
                e = int(max(picks) + max((max(picks) - min(picks)) * tail, sep) + 0.2 * sep)
            else:
                e = max(picks) + 1 + sep
                if sup:
                    e = int(e)
            rec["cut"] = T - len(range(T)[min(T, int(e)):])  # x[:, min(T, int(e)):] = 0, numpy's slicing
            for i in range(n):
                if (sup and e >= T - 2 * sep) or (not sup and e + 2 * sep >= T):
                    break
                if sup:
                    tr, row = rnd.source("event", i, event_traces)
                    sons = onsets[tr] - float(row["start"])
                    P2, S2 = labels_of(sons, T, sigma)
                    if not np.isclose(P2.max(), 1, atol=1e-2):
                        continue
                else:
                    P2, S2 = P, S
                a = int(np.argmax(P2))
                q = rnd.integer("event_q", i, int(e), T - 2 * sep if sup else T - sep)
                d = q - a
                ev = rec["event"][i]
                ev["kind"] = G.AUG_BANK if sup else G.AUG_SELF
                if sup:
                    ev["row"] = row
                ev["zero_before"] = max(a - sep, 0)
                ev["shift"] = max(min(d, T), -T)
                ev["scale"] = 1.0 / rnd.uniform("event_scale", i, 0.25, 4)
                if i != n - 1:
                    end = max(int(np.argmax(shift(P2, d))), int(np.argmax(shift(S2, d)))) + 1 + sep
                    e = max(e, int(end) if sup else end)
    if len(noise_traces):
        br = rnd.branch("noise_branch", noise_prob)
        n = 1 + rnd.branch("n_noise", num)
        if br == 0:
            for j in range(n):
                tr, row = rnd.source("noise", j, noise_traces)
                rec["noise"][j]["kind"] = G.AUG_BANK
                rec["noise"][j]["row"] = row
                rec["noise"][j]["scale"] = 1.0 / rnd.uniform("noise_scale", j, 2, 50)
        elif br == 1:
            rec["gauss"] = rnd.uniform("gauss", None, 0, 0.15)
            if rec["gauss"] > 0:
                rec["noise_key"] = rnd.noise_key()
    if rnd.branch("gap_branch", gap_prob) == 0:
        g0 = rnd.integer("gap_lo", None, 0, T)
        rec["gap_lo"] = g0
        rec["gap_hi"] = rnd.integer("gap_hi", None, g0, T)
    return rec
