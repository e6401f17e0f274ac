"""Plain-loop float64 restatement of csrc/scanrecur.hip for the tests: sp_stats_recurrence_counts and
sp_stats_recurrence_expectation with the documented summation orders, written with Python floats and numpy float64 element-wise
operations (one rounding per operation), and an independent copy of the host statistics written with loops.  Z, D, q, c and the pixel
rule are those of tests/saccade_statistics_ref.py.  Nothing here imports the package."""
import math

import numpy as np

from saccade_statistics_ref import MAX_CELLS, MAX_FIXATIONS, NAN, cell, kept, row_steps  # noqa: F401


def mask(map_shape, frame_size, radius):
    """uint8 [2 Hm - 1, 2 Wm - 1]: 1 iff the pixel length of the displacement is at most radius"""
    Hm, Wm = map_shape
    fh, fw = (float(v) for v in frame_size)
    out = np.zeros((2 * Hm - 1, 2 * Wm - 1), np.uint8)
    for dr in range(-(Hm - 1), Hm):
        for dc in range(-(Wm - 1), Wm):
            dx, dy = dc * fw / Wm, dr * fh / Hm
            out[dr + Hm - 1, dc + Wm - 1] = 1 if math.sqrt(dx * dx + dy * dy) <= radius else 0
    return out


def _line_points(plot, m, L, step):
    """the points of the strict upper triangle of plot [m][m] on lines of at least L points along step = (di, dj)"""
    di, dj = step
    total = 0
    for i in range(m):
        for j in range(i + 1, m):
            before = (i - di, j - dj)
            if not plot[i][j] or (before[0] >= 0 and before[1] > before[0] and plot[before[0]][before[1]]):
                continue                                                 # not the first point of a line
            n, a, b = 0, i, j
            while a < m and b < m and b > a and plot[a][b]:
                n, a, b = n + 1, a + di, b + dj
            if n >= L:
                total += n
    return total


def recurrence_counts(scanpaths, groups, n_groups, frame_size, map_shape, max_steps, table, min_line):
    """-> {"counts" int64 [G, K, K], "points" int32 [S], "dropped" int32 [S], "rqa" int32 [S, 6]}, K = max_steps; table: mask(); a
    scanpath of more than MAX_FIXATIONS fixations or with a group outside [0, n_groups) is refused: points -1, dropped 0, rqa -1"""
    Hm, Wm = map_shape
    fh, fw = (float(v) for v in frame_size)
    S, K = len(scanpaths), max_steps
    counts = np.zeros((n_groups, K, K), np.int64)
    points, drop, rqa = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, 6), np.int32)
    for s, (sp, g) in enumerate(zip(scanpaths, groups)):
        sp = np.asarray(sp, dtype=np.float64)
        if len(sp) > MAX_FIXATIONS or not 0 <= g < n_groups:
            points[s], rqa[s] = -1, -1
            continue
        cells = []
        for i in range(min(len(sp), K)):
            x, y = float(sp[i, 0]), float(sp[i, 1])
            if kept(x, y, fw, fh):
                cells.append((cell(y, Hm, fh), cell(x, Wm, fw)))
            else:
                cells.append(None)
                drop[s] += 1
        m = len(cells)
        plot = [[False] * m for _ in range(m)]
        lag = 0
        for i in range(m):
            if cells[i] is None:
                continue
            counts[g, i, i] += 1
            for j in range(i + 1, m):
                if cells[j] is None:
                    continue
                counts[g, j, i] += 1
                if table[cells[j][0] - cells[i][0] + Hm - 1, cells[j][1] - cells[i][1] + Wm - 1]:
                    plot[i][j] = True
                    counts[g, i, j] += 1
                    points[s] += 1
                    lag += j - i
        rqa[s] = (sum(c is not None for c in cells), points[s], _line_points(plot, m, min_line, (1, 1)),
                  _line_points(plot, m, min_line, (0, 1)), _line_points(plot, m, min_line, (1, 0)), lag)
    return {"counts": counts, "points": points, "dropped": drop, "rqa": rqa}


def measures(rqa):
    """REC, DET, LAM, CORM of one row of integers, by the formulas of Anderson et al. 2013"""
    N, R, DL, HL, VL, lag = (int(v) for v in rqa)
    return {"REC": 100.0 * 2 * R / (N * (N - 1)) if N >= 2 else NAN, "DET": 100.0 * DL / R if R else NAN,
            "LAM": 100.0 * (HL + VL) / (2 * R) if R else NAN, "CORM": 100.0 * lag / ((N - 1) * R) if R and N >= 2 else NAN}


def lane_sum(values):
    """saccade_statistics_ref.lane_sum on an array: lane l adds elements l, l + 64, .. from 0.0 (rows of 64 added one after another;
    the zeros that pad the last row change nothing), then the xor butterfly 32 .. 1"""
    v = np.asarray(values, dtype=np.float64)
    v = np.concatenate([v, np.zeros(-len(v) % 64)]).reshape(-1, 64)
    part = np.zeros(64)
    for row in v:
        part = part + row
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ o]
    return float(part[0])


def blur(c, table):
    """B(i) = the sum of c(i + d) over the displacements d with a non-zero table entry whose partner lies inside the map, d in
    ascending lattice index from 0.0: one element-wise addition per d keeps that order for every cell"""
    LH, LW = table.shape
    Hm, Wm = (LH + 1) // 2, (LW + 1) // 2
    grid, B = np.asarray(c, dtype=np.float64).reshape(Hm, Wm), np.zeros((Hm, Wm))
    for dr in range(-(Hm - 1), Hm):
        for dc in range(-(Wm - 1), Wm):
            if table[dr + Hm - 1, dc + Wm - 1]:
                r0, r1, c0, c1 = max(0, -dr), min(Hm, Hm - dr), max(0, -dc), min(Wm, Wm - dc)
                B[r0:r1, c0:c1] = B[r0:r1, c0:c1] + grid[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return B.reshape(-1)


def row_expectation(p_row, table, min_length, max_steps):
    """(E_r float64 [Tm, Tm], points, bad) of one row, Tm = min(T, max_steps)"""
    Tm = min(len(p_row), max_steps)
    E = np.zeros((Tm, Tm))
    steps = row_steps(p_row, min_length, Tm)
    if steps is None:
        return E, NAN, 1
    c, q = steps
    A = [1.0]
    for u in range(Tm):
        A.append(A[u] * (1.0 - q[u]))
    for t in range(Tm):
        B = blur(c[t], table)
        E[t, t] = A[t] * (1.0 - q[t])
        for s in range(t):
            x = lane_sum(c[s] * B)
            G = 1.0
            for u in range(s + 1, t):
                G = G * (1.0 - q[u])
            AG = A[s] * G
            E[s, t] = AG * x
            E[t, s] = AG * ((1.0 - q[s]) * (1.0 - q[t]))
    points = 0.0
    for s in range(Tm):
        for t in range(s + 1, Tm):
            points = points + float(E[s, t])
    return E, points, 0


def recurrence_expectation(probs, row_groups, n_groups, table, min_length, max_steps, rows=None):
    """probs float32 [R, T, 1 + P] -> {"E" float64 [G, K, K], "points" float64 [R], "bad" int32 [R], "rows": the per-row (E_r, points,
    bad), to be passed back as rows= with other groups}"""
    probs = np.asarray(probs, dtype=np.float32)
    R, K = probs.shape[0], max_steps
    assert probs.shape[2] - 1 == (table.shape[0] + 1) // 2 * ((table.shape[1] + 1) // 2) <= MAX_CELLS and 1 <= K <= MAX_FIXATIONS
    E = np.zeros((n_groups, K, K))
    points, bad = np.full(R, NAN), np.zeros(R, np.int32)
    per_row = [None] * R if rows is None else rows
    for r in range(R):                                                   # ascending row index
        g = int(row_groups[r])
        if not 0 <= g < n_groups:
            bad[r] = -1
            continue
        if per_row[r] is None:
            per_row[r] = row_expectation(probs[r], table, min_length, max_steps)
        Er, p, b = per_row[r]
        points[r], bad[r] = p, b
        if b == 0:
            Tm = Er.shape[0]
            E[g, :Tm, :Tm] = E[g, :Tm, :Tm] + Er
    return {"E": E, "points": points, "bad": bad, "rows": per_row}


# ---- the host statistics, written independently (loops) ---------------------------------------------------------------------------------
def summary(table):
    table = np.asarray(table, dtype=np.float64)
    K = table.shape[0]
    fix = pairs = points = lag_up = lag_low = 0.0
    up, low = [0.0] * (K - 1), [0.0] * (K - 1)
    for s in range(K):
        fix += float(table[s, s])
        for t in range(s + 1, K):
            points += float(table[s, t])
            pairs += float(table[t, s])
            up[t - s - 1] += float(table[s, t])
            low[t - s - 1] += float(table[t, s])
            lag_up += (t - s) * float(table[s, t])
            lag_low += (t - s) * float(table[t, s])
    return {"fixations": fix, "pairs": pairs, "points": points, "REC": 100.0 * points / pairs if pairs > 0 else NAN,
            "recurrence_by_lag": [u / v if v > 0 else NAN for u, v in zip(up, low)],
            "mean_lag": lag_up / points if points > 0 else NAN, "mean_lag_chance": lag_low / pairs if pairs > 0 else NAN}
