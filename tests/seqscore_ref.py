"""Checker of csrc/seqscore.hip: flat-kernel mean shift, cluster-label strings, the sequence score (Needleman-Wunsch
with the 0/1 similarity, divided by the longer length) and the fixation edit distance (Levenshtein), written from the definitions as
plain Python loops over IEEE doubles: every difference, product, sum, square root and division is one rounded double operation (Python
floats: no extended precision, no fused multiply-add), sums run left to right in index order, starting from 0.0.

meanshift_loops is the definition, loop by loop.  meanshift states the same arithmetic with numpy for the element-wise part (numpy's
subtract / multiply / add / less_equal are the same single IEEE operations) and np.add.accumulate for the sums, which adds strictly
left to right (np.sum does not: it sums pairwise); tests/test_sequence_score_cpu.py holds the two bit-identical.  It is what the GPU
tests use, because the loops take minutes on a thousand points."""
import math

import numpy as np

NAN = float("nan")
METRICS = ("SS", "FED")
MAX_FIXATIONS = 64


def _xy(points):
    a = np.asarray(points, dtype=np.float64)
    a = a.reshape(len(a), -1) if len(a) else np.zeros((0, 2))
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])


def _seed_loops(xs, ys, s, h2, stop, max_iter):
    """(k, cx, cy) of seed s, or None if a neighbourhood is empty"""
    cx, cy = xs[s], ys[s]
    it = 0
    while True:
        sx, sy, k = 0.0, 0.0, 0
        for x, y in zip(xs, ys):
            dx = x - cx
            dy = y - cy
            if dx * dx + dy * dy <= h2:
                sx = sx + x
                sy = sy + y
                k += 1
        if k == 0:
            return None
        nx, ny = sx / float(k), sy / float(k)
        dx, dy = nx - cx, ny - cy
        cx, cy = nx, ny
        if math.sqrt(dx * dx + dy * dy) <= stop or it == max_iter:
            return k, cx, cy
        it += 1


def _seed_numpy(X, Y, s, h2, stop, max_iter):
    cx, cy = X[s], Y[s]
    it = 0
    while True:
        dx = X - cx
        dy = Y - cy
        inside = dx * dx + dy * dy <= h2
        k = int(np.count_nonzero(inside))
        if k == 0:
            return None
        # 0.0 + x0 + x1 + ..., strictly left to right (0.0 + x0 == x0 except for x0 = -0.0, which becomes +0.0 either way below)
        sx = np.add.accumulate(X[inside])[-1] + 0.0
        sy = np.add.accumulate(Y[inside])[-1] + 0.0
        nx, ny = sx / np.float64(k), sy / np.float64(k)
        dx, dy = nx - cx, ny - cy
        cx, cy = nx, ny
        if math.sqrt(dx * dx + dy * dy) <= stop or it == max_iter:
            return k, float(cx), float(cy)
        it += 1


def _clusters(entries, h2):
    """entries: (k, cx, cy, seed) of the seeds that yielded one -> (centres [K, 2], weight [K])"""
    order = sorted(entries, key=lambda e: (-e[0], -e[1], -e[2], e[3]))
    gone = [False] * len(order)
    centres, weight = [], []
    for a, (k, cx, cy, _) in enumerate(order):
        if gone[a]:
            continue
        centres.append((cx, cy))
        weight.append(k)
        for b in range(a + 1, len(order)):
            dx = order[b][1] - cx
            dy = order[b][2] - cy
            if dx * dx + dy * dy <= h2:
                gone[b] = True
    return np.array(centres, dtype=np.float64).reshape(-1, 2), np.array(weight, dtype=np.int32)


def labels_of(points, centres):
    """int32 [n]: the centre with the smallest dx*dx + dy*dy, the lowest index on ties; -1 everywhere when there is no centre"""
    xs, ys = _xy(points)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    out = np.full(len(xs), -1, dtype=np.int32)
    if len(centres) == 0:
        return out
    for i, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
        best, lab = None, -1
        for k, (cx, cy) in enumerate(centres.tolist()):
            dx = x - cx
            dy = y - cy
            d = dx * dx + dy * dy
            if k == 0 or d < best:
                best, lab = d, k
        out[i] = lab
    return out


def _meanshift(points, bandwidth, max_iter, seed_fn, as_lists):
    X, Y = _xy(points)
    h = float(bandwidth)
    h2, stop = h * h, 1e-3 * h
    xs, ys = (X.tolist(), Y.tolist()) if as_lists else (X, Y)
    entries = []
    for s in range(len(X)):
        r = seed_fn(xs, ys, s, h2, stop, int(max_iter))
        if r is not None:
            entries.append((r[0], r[1], r[2], s))
    centres, weight = _clusters(entries, h2)
    return centres, weight, labels_of(points, centres)


def meanshift_loops(points, bandwidth, max_iter=300):
    """(centres [K, 2] float64, weight [K] int32, labels [n] int32) of one group: the definition, in plain loops"""
    return _meanshift(points, bandwidth, max_iter, _seed_loops, True)


def meanshift(points, bandwidth, max_iter=300):
    """the same bits as meanshift_loops, quicker (see the module docstring)"""
    return _meanshift(points, bandwidth, max_iter, _seed_numpy, False)


def predict(points, centres):
    return labels_of(points, centres)


def _max(a, b):
    return b if b > a else a


def nw_table_end(a, b, gap=0.0):
    """F[n][m] of the Needleman-Wunsch table with similarity 1.0 / 0.0 and a linear gap"""
    n, m = len(a), len(b)
    gap = float(gap)
    F = [[0.0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        F[i][0] = gap * float(i)
    for j in range(m + 1):
        F[0][j] = gap * float(j)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            F[i][j] = _max(_max(F[i - 1][j - 1] + (1.0 if a[i - 1] == b[j - 1] else 0.0), F[i - 1][j] + gap), F[i][j - 1] + gap)
    return F[n][m]


def _refused(a, b):
    return len(a) > MAX_FIXATIONS or len(b) > MAX_FIXATIONS or any(int(v) < 0 for v in a) or any(int(v) < 0 for v in b)


def sequence_score(a, b, gap=0.0):
    a, b = [int(v) for v in a], [int(v) for v in b]
    if _refused(a, b) or max(len(a), len(b)) == 0:
        return NAN
    return nw_table_end(a, b, gap) / float(max(len(a), len(b)))


def fixation_edit_distance(a, b):
    a, b = [int(v) for v in a], [int(v) for v in b]
    if _refused(a, b):
        return NAN
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return float(D[n][m])


def lcs(a, b):
    n, m = len(a), len(b)
    T = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            T[i][j] = T[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(T[i - 1][j], T[i][j - 1])
    return T[n][m]


def score_pairs(strings, pairs, metrics=METRICS, gap=0.0):
    """{metric: float64 [npairs]} for pairs[p] = (index of a, index of b)"""
    out = {m: np.zeros(len(pairs), dtype=np.float64) for m in metrics}
    for p, (i, j) in enumerate(pairs):
        if "SS" in out:
            out["SS"][p] = sequence_score(strings[int(i)], strings[int(j)], gap)
        if "FED" in out:
            out["FED"][p] = fixation_edit_distance(strings[int(i)], strings[int(j)])
    return out
