"""The definitions of DESIGN.md §19 in plain Python / numpy loops, float64: human scanpaths under a model's per-step distributions.
It takes the same float32 probabilities as the device (every p enters as the float32 value converted exactly to float64), shares no
code with the package, and sums serially in index order -- the device sums lane-strided with a butterfly, so the two agree to a few
ulp, not bit for bit (tests/test_scanpath_likelihood_gpu.py states the bar); the integer quantities (AUC, n, dropped) are exact.

    res = scanpath_likelihood(probs, scanpaths, rows, frame_size, map_shape, uniform_mix=0.0, baseline=None, baseline_rows=None,
                              mu=None, sigma2=None, min_length=0, quick=False)
    # {"LL", "IG", "NSS", "AUC", "DLL": [S, T], "STOP": [S], "CONT", "TERM": [R, T], "n", "dropped": int32 [S]}

quick=True replaces the serial sums by numpy's (pairwise) sums: the host path a user without the device would write; it is what
tests/diagnostics/bench_scanpath_likelihood.py times."""
import math

import numpy as np

METRICS = ("LL", "IG", "NSS", "AUC", "DLL", "STOP")
MAX_FIXATIONS = 64
MAX_CELLS = 2048
NAN = float("nan")
F = np.float64


def cell_of(x, y, frame_size, map_shape):
    """the cell index row * Wm + col of a fixation (the pixel rule of fixation_maps), None for a dropped one"""
    h, w = (float(v) for v in frame_size)
    Hm, Wm = map_shape
    x, y = float(x), float(y)
    if not (math.isfinite(x) and math.isfinite(y)) or x < 0.0 or x >= w or y < 0.0 or y >= h:
        return None
    col = min(int(math.floor((x * Wm) / w)), Wm - 1)
    row = min(int(math.floor((y * Hm) / h)), Hm - 1)
    return row * Wm + col


def _sum(values, quick):
    if quick:
        return F(np.sum(np.asarray(values, dtype=np.float64)))
    acc = F(0.0)
    for v in values:
        acc = acc + v
    return acc


def step_stats(p, quick=False):
    """p float32 [1 + P] -> (Z, mean, std or NaN, CONT, TERM)"""
    p = np.asarray(p)
    assert p.dtype == np.float32
    cells = p[1:].astype(np.float64)                     # exact
    P = len(cells)
    with np.errstate(all="ignore"):
        Z = _sum(cells, quick)
        mean = Z / F(P)
        std = F(NAN)
        if P >= 2 and p[1:].min() != p[1:].max():         # the raw float32 minimum and maximum decide, not the variance
            squares = (cells - mean) * (cells - mean) if quick else [(c - mean) * (c - mean) for c in cells]
            std = np.sqrt(_sum(squares, quick) / F(P - 1))
        p0 = F(p[0])
        return Z, mean, std, np.log2(Z / (Z + p0)), np.log2(p0 / (Z + p0))


def duration_log2_density(d, mu, s2):
    d, mu, s2 = F(d), F(mu), F(s2)
    if not (d > 0 and np.isfinite(d) and s2 > 0):
        return F(NAN)
    with np.errstate(all="ignore"):
        ld = np.log(d)
        e = ld - mu
        return (-ld - F(0.5) * np.log(F(2.0) * F(math.pi) * s2) - e * e / (F(2.0) * s2)) / F(math.log(2.0))


def stop_log2_probability(cont, term, n, min_length):
    """cont, term [T] of the scanpath's row; n = min(len, T)"""
    T = len(cont)
    if n < min_length and n < T:
        return F(-np.inf)
    acc = F(0.0)
    for t in range(min_length, n):
        acc = acc + cont[t]
    if n < T:
        acc = acc + term[n]
    return acc


def scanpath_likelihood(probs, scanpaths, rows, frame_size, map_shape, uniform_mix=0.0, baseline=None, baseline_rows=None, mu=None,
                        sigma2=None, min_length=0, quick=False):
    probs = np.asarray(probs)
    assert probs.dtype == np.float32 and probs.ndim == 3
    R, T, A = probs.shape
    Hm, Wm = map_shape
    P = Hm * Wm
    assert A == P + 1 and P <= MAX_CELLS
    S = len(scanpaths)
    u = F(uniform_mix)
    out = {m: np.full((S, T), NAN) for m in METRICS[:5]}
    out["STOP"] = np.full(S, NAN)
    out["CONT"], out["TERM"] = np.full((R, T), NAN), np.full((R, T), NAN)
    out["n"], out["dropped"] = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    stats = {}
    for r in range(R):
        for t in range(T):
            stats[r, t] = step_stats(probs[r, t], quick)
            out["CONT"][r, t], out["TERM"][r, t] = stats[r, t][3:]
    bsum = None
    if baseline is not None:
        baseline = np.asarray(baseline, dtype=np.float64)
        bsum = [_sum(b, quick) for b in baseline]
    with np.errstate(all="ignore"):
        for s, sp in enumerate(scanpaths):
            sp = np.asarray(sp, dtype=np.float64)
            assert len(sp) <= MAX_FIXATIONS
            r = int(rows[s])
            n = min(len(sp), T)
            out["n"][s] = n
            out["STOP"][s] = stop_log2_probability(out["CONT"][r], out["TERM"][r], n, min_length)
            for t in range(n):
                if mu is not None and sp.shape[1] >= 3:
                    out["DLL"][s, t] = duration_log2_density(sp[t, 2], np.asarray(mu)[r, t], np.asarray(sigma2)[r, t])
                c = cell_of(sp[t, 0], sp[t, 1], frame_size, map_shape)
                if c is None:
                    out["dropped"][s] += 1
                    continue
                Z, mean, std = stats[r, t][:3]
                raw = probs[r, t, 1:]
                pc = F(raw[c])
                q = (F(1.0) - u) * (pc / Z) + u / F(P)
                out["LL"][s, t] = np.log2(F(P) * q)
                out["NSS"][s, t] = (pc - mean) / std
                if P >= 2:
                    below, equal = int((raw < raw[c]).sum()), int((raw == raw[c]).sum())      # integers: order-free
                    out["AUC"][s, t] = (F(below) + F(0.5) * F(equal - 1)) / F(P - 1)
                if baseline is not None:
                    b = int(baseline_rows[s])
                    if bsum[b] > 0:
                        out["IG"][s, t] = np.log2(q) - np.log2((F(1.0) - u) * (baseline[b, c] / bsum[b]) + u / F(P))
    return out
