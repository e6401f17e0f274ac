"""The yardstick of the shuffled AUC, CC, SIM and information gain (csrc/salmaps.hip sp_saliency_scores, sp_fixation_pool_counts): a
numpy restatement of the published formulae (Bylinskii et al., TPAMI 2019) on sum-normalised maps, float64, written for the tests --
the reference has no counterpart.  Per map of P pixels: S the predicted density, F the fixation map (fixated where F > 0), D the human
density, Bm the baseline density, w the integer pool weights.

    cnt, tot = pool_counts(F [G,...], cls [G], E)       # cnt[e][p] = #(maps h of image e with F_h[p] > 0), tot = cnt.sum(0)
    w = pool_weights(cnt, tot, cls)                      # w[g] = tot - cnt[cls[g]]
    sauc(S, F, w)   cc(S, D)   sim(S, D)   infogain(S, F, Bm, uniform_mix)

sauc is the exact weighted Mann-Whitney AUC in its sorted form; sauc_brute loops over the fixated pixels, and sauc(..., brute=True)
asserts that the two agree to the bit (both divide the same integers)."""
import numpy as np

EPS = 2.220446049250313e-16


def pool_counts(F, cls, E):
    F = np.asarray(F)
    cnt = np.zeros((E,) + F.shape[1:], dtype=np.int64)
    for f, e in zip(F, cls):
        cnt[int(e)] += f > 0
    return cnt, cnt.sum(0)


def pool_weights(cnt, tot, cls):
    return np.stack([tot - cnt[int(e)] for e in cls])


def _sauc_parts(S, F, w):
    S, F, w = np.asarray(S, dtype=np.float64).ravel(), np.asarray(F).ravel(), np.asarray(w).ravel().astype(np.int64)
    w = np.where(w > 0, w, 0)
    return S, F > 0, w


def sauc_brute(S, F, w):
    S, pos, w = _sauc_parts(S, F, w)
    n, W = int(pos.sum()), int(w.sum())
    if n == 0 or W == 0 or np.isnan(S).any():
        return float("nan")
    num = 0
    for i in np.flatnonzero(pos):
        num += 2 * int((w * (S < S[i])).sum()) + int((w * (S == S[i])).sum())
    return float(num) / float(2 * n * W)


def sauc(S, F, w, brute=False):
    S, pos, w = _sauc_parts(S, F, w)
    n, W = int(pos.sum()), int(w.sum())
    if n == 0 or W == 0 or np.isnan(S).any():
        out = float("nan")
    else:
        t = np.sort(S[pos])
        m = w > 0
        above = n - np.searchsorted(t, S[m], side="right")               # fixated values > the pool pixel's
        at_or_above = n - np.searchsorted(t, S[m], side="left")
        num = int((w[m] * (above + at_or_above)).sum())                  # = sum over fixated i of 2 below_i + equal_i
        out = float(num) / float(2 * n * W)
    if brute:
        b = sauc_brute(S, F, w)
        assert (np.isnan(out) and np.isnan(b)) or out == b, (out, b)
    return out


def cc(S, D):
    S, D = np.asarray(S, dtype=np.float64).ravel(), np.asarray(D, dtype=np.float64).ravel()
    with np.errstate(all="ignore"):
        a, b = S - S.mean(), D - D.mean()
        xx, yy = (a * a).sum(), (b * b).sum()
        if not (np.isfinite(xx) and np.isfinite(yy)) or xx == 0 or yy == 0:
            return float("nan")
        return float((a * b).sum() / np.sqrt(xx * yy))


def _sum_ok(x):
    return bool(np.isfinite(x) and x > 0)


def sim(S, D):
    S, D = np.asarray(S, dtype=np.float64).ravel(), np.asarray(D, dtype=np.float64).ravel()
    with np.errstate(all="ignore"):
        sS, sD = S.sum(), D.sum()
        if not (_sum_ok(sS) and _sum_ok(sD)):
            return float("nan")
        return float(np.minimum(S / sS, D / sD).sum())


def infogain(S, F, Bm, uniform_mix):
    S, Bm = np.asarray(S, dtype=np.float64).ravel(), np.asarray(Bm, dtype=np.float64).ravel()
    pos = np.asarray(F).ravel() > 0
    with np.errstate(all="ignore"):
        sS, sB = S.sum(), Bm.sum()
        if not pos.any() or not (_sum_ok(sS) and _sum_ok(sB)):
            return float("nan")
        a, P = float(uniform_mix), S.size
        p = (1.0 - a) * S / sS + a / P
        q = (1.0 - a) * Bm / sB + a / P
        return float((np.log2(EPS + p[pos]) - np.log2(EPS + q[pos])).mean())
