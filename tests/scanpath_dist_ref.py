"""Checker of csrc/scandist.hip: dynamic time warping, the discrete Frechet distance, the Hausdorff distance, Eyenalysis
(position only) and the cross-recurrence measures REC / DET / LAM / CORM, as plain Python double loops over IEEE doubles in exactly the
order of operations the definitions state -- every product, sum, square root and division is one rounded double operation (Python
floats: no extended precision, no fused multiply-add; math.sqrt is the correctly rounded square root), sums run left to right in index
order.  P is the first (human) scanpath, Q the second; only columns 0 and 1 are read; coordinates are divided by max_dim first."""
import math

import numpy as np

DISTANCES = ("DTW", "Frechet", "Hausdorff", "Eyenalysis")
RECURRENCE = ("REC", "DET", "LAM", "CORM")
NAN = float("nan")


def _xy(path, max_dim):
    a = np.asarray(path, dtype=np.float64)
    a = a.reshape(len(a), -1) if len(a) else np.zeros((0, 2))
    md = float(max_dim)
    return [(float(r[0]) / md, float(r[1]) / md) for r in a]


def dist_matrix(P, Q, max_dim=1.0):
    """(d, n, m): d[i][j] = sqrt(dx*dx + dy*dy) of P_i and Q_j, a list of rows of Python floats"""
    p, q = _xy(P, max_dim), _xy(Q, max_dim)
    d = []
    for px, py in p:
        row = []
        for qx, qy in q:
            dx, dy = px - qx, py - qy
            row.append(math.sqrt(dx * dx + dy * dy))
        d.append(row)
    return d, len(p), len(q)


def _sweep(d, n, m, join):
    D = [[None] * m for _ in range(n)]
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[i][j] = d[0][0]
            elif j == 0:
                D[i][j] = join(D[i - 1][0], d[i][0])
            elif i == 0:
                D[i][j] = join(D[0][j - 1], d[0][j])
            else:
                D[i][j] = join(min(D[i - 1][j - 1], D[i - 1][j], D[i][j - 1]), d[i][j])
    return float(D[n - 1][m - 1])


def _dtw(d, n, m):
    return NAN if n == 0 or m == 0 else _sweep(d, n, m, lambda a, b: a + b)


def _frechet(d, n, m):
    return NAN if n == 0 or m == 0 else _sweep(d, n, m, max)


def _hausdorff(d, n, m):
    if n == 0 or m == 0:
        return NAN
    return max(max(min(d[i][j] for j in range(m)) for i in range(n)), max(min(d[i][j] for i in range(n)) for j in range(m)))


def _eyenalysis(d, n, m):
    if n == 0 or m == 0:
        return NAN
    s = 0.0
    for i in range(n):
        s = s + min(d[i][j] for j in range(m))
    for j in range(m):
        s = s + min(d[i][j] for i in range(n))
    return s / float(max(n, m))


def dtw(P, Q, max_dim=1.0):
    return _dtw(*dist_matrix(P, Q, max_dim))


def frechet(P, Q, max_dim=1.0):
    return _frechet(*dist_matrix(P, Q, max_dim))


def hausdorff(P, Q, max_dim=1.0):
    return _hausdorff(*dist_matrix(P, Q, max_dim))


def eyenalysis(P, Q, max_dim=1.0):
    return _eyenalysis(*dist_matrix(P, Q, max_dim))


def _run_points(line, L):
    """how many set entries of a 0/1 sequence lie on runs of at least L"""
    total = run = 0
    for c in list(line) + [0]:
        if c:
            run += 1
        else:
            if run >= L:
                total += run
            run = 0
    return total


def cross_recurrence(P, Q, radius, min_line=2, max_dim=1.0):
    """(REC, DET, LAM, CORM) in per cent; Anderson et al. 2015, the cross-recurrence form over the full N x N matrix"""
    return _recurrence(*dist_matrix(P, Q, max_dim), radius, min_line)


def _recurrence(d, n, m, radius, min_line):
    N, L = min(n, m), int(min_line)
    if N == 0:
        return (NAN,) * 4
    rad = float(radius)
    c = [[1 if d[i][j] <= rad else 0 for j in range(N)] for i in range(N)]
    R = sum(sum(row) for row in c)
    rec = 100.0 * float(R) / float(N * N)
    if R == 0:
        return rec, NAN, NAN, NAN
    DL = sum(_run_points([c[i][i + k] for i in range(N) if 0 <= i + k < N], L) for k in range(-(N - 1), N))
    HL = sum(_run_points(c[i], L) for i in range(N))
    VL = sum(_run_points([c[i][j] for i in range(N)], L) for j in range(N))
    S = sum((j - i) * c[i][j] for i in range(N) for j in range(N))
    det = 100.0 * float(DL) / float(R)
    lam = 100.0 * float(HL + VL) / float(2 * R)
    corm = NAN if N == 1 else 100.0 * float(S) / float((N - 1) * R)
    return rec, det, lam, corm


_FN = {"DTW": _dtw, "Frechet": _frechet, "Hausdorff": _hausdorff, "Eyenalysis": _eyenalysis}


def score_pairs(scanpaths, pairs, metrics, max_dim=1.0, radius=None, min_line=2):
    """dict of float64 [npairs] arrays: what scanpath_distances_pairs returns, from the loops above"""
    pairs = [tuple(int(v) for v in p) for p in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)]
    out = {m: np.full(len(pairs), np.nan) for m in metrics}
    want_rec = [m for m in metrics if m in RECURRENCE]
    for k, (a, b) in enumerate(pairs):
        dnm = dist_matrix(scanpaths[a], scanpaths[b], max_dim)             # once per pair
        for m in metrics:
            if m in _FN:
                out[m][k] = _FN[m](*dnm)
        if want_rec:
            r = _recurrence(*dnm, radius, min_line)
            for m in want_rec:
                out[m][k] = r[RECURRENCE.index(m)]
    return out
