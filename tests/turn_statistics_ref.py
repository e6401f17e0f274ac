"""Plain-loop float64 restatement of csrc/scanturn.hip for the tests: sp_scan_turn_counts and sp_scan_turn_expectation
with the documented summation orders, written with Python floats and numpy float64 element-wise operations (one rounding per
operation), the closed form again without any summation order (rationals, numpy's extended precision), and an independent copy of the
host statistics written with loops.  Z, D, q, c and the pixel rule are those of tests/saccade_statistics_ref.py.  Nothing here imports
the package."""
import math
from fractions import Fraction

import numpy as np

from saccade_statistics_ref import MAX_CELLS, MAX_FIXATIONS, NAN, cell, jensen_shannon, kept, row_steps  # noqa: F401

MAX_DIRECTIONS = 16


def sectors(map_shape, frame_size, n):
    """int32 [2 Hm - 1, 2 Wm - 1]: sector floor(atan2(dy, dx) * n / (2 pi) + 0.5) mod n of every displacement in pixels, n for the zero
    displacement"""
    Hm, Wm = map_shape
    fh, fw = (float(v) for v in frame_size)
    out = np.zeros((2 * Hm - 1, 2 * Wm - 1), np.int32)
    for dr in range(-(Hm - 1), Hm):
        for dc in range(-(Wm - 1), Wm):
            dx, dy = dc * fw / Wm, dr * fh / Hm
            out[dr + Hm - 1, dc + Wm - 1] = n if dr == 0 and dc == 0 else int(math.floor(math.atan2(dy, dx) * n / (2 * math.pi) + 0.5)) % n
    return out


def turn_counts(scanpaths, groups, n_groups, frame_size, map_shape, max_steps, sector):
    """-> {"counts" int64 [G, n + 1, n + 1], "pairs" int32 [S], "dropped" int32 [S]}; sector: the table of sectors() (n is read off the
    caller's n_directions = sector's largest possible value, passed as its zero entry); a scanpath of more than MAX_FIXATIONS fixations
    or with a group outside [0, n_groups) is refused: pairs -1, dropped 0, nothing counted"""
    Hm, Wm = map_shape
    fh, fw = (float(v) for v in frame_size)
    n = int(sector[Hm - 1, Wm - 1])
    S = len(scanpaths)
    counts = np.zeros((n_groups, n + 1, n + 1), np.int64)
    pairs, drop = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s, (sp, g) in enumerate(zip(scanpaths, groups)):
        sp = np.asarray(sp, dtype=np.float64)
        if len(sp) > MAX_FIXATIONS or not 0 <= g < n_groups:
            pairs[s] = -1
            continue
        cells = []
        for i in range(min(len(sp), max_steps)):
            x, y = float(sp[i, 0]), float(sp[i, 1])
            if kept(x, y, fw, fh):
                cells.append((cell(y, Hm, fh), cell(x, Wm, fw)))
            else:
                cells.append(None)
                drop[s] += 1
        for a, b, c in zip(cells[:-2], cells[1:-1], cells[2:]):
            if a is not None and b is not None and c is not None:
                counts[g, sector[b[0] - a[0] + Hm - 1, b[1] - a[1] + Wm - 1], sector[c[0] - b[0] + Hm - 1, c[1] - b[1] + Wm - 1]] += 1
                pairs[s] += 1
    return {"counts": counts, "pairs": pairs, "dropped": drop}


def fan(c, sector, incoming):
    """float64 [P, n + 1]: incoming: fan[b][k] = sum of c(a) over the cells a with sector(b - a) = k; else over those with
    sector(a - b) = k.  The kernel's order: for every b the cells a in ascending row-major order from 0.0 -- looping over a and adding
    c(a) to ONE bin of every b keeps that order for every (b, k)."""
    LH, LW = sector.shape
    Hm, Wm = (LH + 1) // 2, (LW + 1) // 2
    P, n = Hm * Wm, int(sector[Hm - 1, Wm - 1])
    table = sector if incoming else sector[::-1, ::-1]              # sector(a - b) sits at the mirror image of sector(b - a)
    out = np.zeros((P, n + 1))
    every = np.arange(P)
    for a in range(P):
        ra, ca = divmod(a, Wm)
        which = table[Hm - 1 - ra:2 * Hm - 1 - ra, Wm - 1 - ca:2 * Wm - 1 - ca].reshape(-1)       # entry b: sector(b - a)
        out[every, which] += c[a]
    return out


def triple_table(c0, c1, c2, sector):
    """X[k][k'] = sum over the cells b, in ascending b from 0.0, of (c1(b) * in[b][k]) * out[b][k'], each product rounded"""
    fin, fout = fan(c0, sector, True), fan(c2, sector, False)
    X = np.zeros((fin.shape[1], fin.shape[1]))
    for b in range(len(c1)):
        X = X + (c1[b] * fin[b])[:, None] * fout[b][None, :]
    return X


def row_expectation(p_row, sector, min_length, max_steps):
    """(M_r float64 [n + 1, n + 1], pairs, bad) of one row"""
    n = int(sector[sector.shape[0] // 2, sector.shape[1] // 2])
    Tm = min(len(p_row), max_steps)
    M = np.zeros((n + 1, n + 1))
    steps = row_steps(p_row, min_length, Tm)
    if steps is None:
        return M, NAN, 1
    c, q = steps
    A, total = 1.0, 0.0
    for t in range(Tm - 2):
        M = M + A * triple_table(c[t], c[t + 1], c[t + 2], sector)
        total = total + A * (((1.0 - q[t]) * (1.0 - q[t + 1])) * (1.0 - q[t + 2]))
        A = A * (1.0 - q[t])
    return M, total, 0


def turn_expectation(probs, row_groups, n_groups, sector, min_length, max_steps, rows=None):
    """probs float32 [R, T, 1 + P] -> {"M" float64 [G, n + 1, n + 1], "pairs" float64 [R], "bad" int32 [R], "rows": the per-row
    (M_r, pairs, bad), to be passed back as rows= with other groups}"""
    probs = np.asarray(probs, dtype=np.float32)
    R = probs.shape[0]
    n = int(sector[sector.shape[0] // 2, sector.shape[1] // 2])
    assert probs.shape[2] - 1 == (sector.shape[0] + 1) // 2 * ((sector.shape[1] + 1) // 2) <= MAX_CELLS and 1 <= n <= MAX_DIRECTIONS
    M = np.zeros((n_groups, n + 1, n + 1))
    pairs, bad = np.full(R, NAN), np.zeros(R, np.int32)
    per_row = [None] * R if rows is None else rows
    for r in range(R):                                                   # ascending row index
        g = int(row_groups[r])
        if not 0 <= g < n_groups:
            bad[r] = -1
            continue
        if per_row[r] is None:
            per_row[r] = row_expectation(probs[r], sector, min_length, max_steps)
        Mr, s, b = per_row[r]
        pairs[r], bad[r] = s, b
        if b == 0:
            M[g] = M[g] + Mr
    return {"M": M, "pairs": pairs, "bad": bad, "rows": per_row}


def _steps_any(p_row, min_length, Tm, doubles, number, total):
    """(c [Tm][P], q [Tm]) in the arithmetic of `number`: doubles=True: the DOUBLES of row_steps (the kernel's Z order and divisions)
    taken as the numbers they are; else from the float32 inputs without any rounding order"""
    if doubles:
        cd, qd = row_steps(p_row, min_length, Tm)
        return [[number(float(v)) for v in row] for row in cd], [number(float(v)) for v in qd]
    c, q = [], []
    for t in range(Tm):
        cells = [number(float(v)) for v in p_row[t][1:]]
        p0 = number(float(p_row[t][0])) if t >= min_length else number(0)
        D = total(cells) + p0
        c.append([v / D for v in cells])
        q.append(p0 / D)
    return c, q


def row_expectation_exact(p_row, sector, min_length, max_steps, doubles=False):
    """The closed form of a good row without any summation order, in rationals; only the results are rounded to double.
    -> (M_r float64 [n + 1, n + 1], pairs).  About 2 P^2 T rational additions: for small maps only."""
    LH, LW = sector.shape
    Hm, Wm = (LH + 1) // 2, (LW + 1) // 2
    P, n = Hm * Wm, int(sector[Hm - 1, Wm - 1])
    Tm = min(len(p_row), max_steps)
    c, q = _steps_any(p_row, min_length, Tm, doubles, Fraction, sum)
    sec = [[int(sector[b // Wm - a // Wm + Hm - 1, b % Wm - a % Wm + Wm - 1]) for a in range(P)] for b in range(P)]   # [b][a]: b - a
    M = [[Fraction(0)] * (n + 1) for _ in range(n + 1)]
    A, total = Fraction(1), Fraction(0)
    for t in range(Tm - 2):
        for b in range(P):
            fin, fout = [Fraction(0)] * (n + 1), [Fraction(0)] * (n + 1)
            for a in range(P):
                fin[sec[b][a]] += c[t][a]
                fout[sec[a][b]] += c[t + 2][a]
            w = A * c[t + 1][b]
            for k in range(n + 1):
                for kk in range(n + 1):
                    M[k][kk] += w * fin[k] * fout[kk]
        total += A * (1 - q[t]) * (1 - q[t + 1]) * (1 - q[t + 2])
        A *= 1 - q[t]
    return np.array([[float(v) for v in row] for row in M]), float(total)


def row_expectation_wide(p_row, sector, min_length, max_steps, doubles=False):
    """The same in numpy's extended precision (np.longdouble, 64 significant bits on x86: 2^-11 of a double's rounding per operation)
    and in another order (masked pairwise sums per sector, one matrix product over b) -- for maps too large for rationals"""
    LH, LW = sector.shape
    Hm, Wm = (LH + 1) // 2, (LW + 1) // 2
    P, n = Hm * Wm, int(sector[Hm - 1, Wm - 1])
    Tm = min(len(p_row), max_steps)
    wide = np.longdouble
    c, q = _steps_any(p_row, min_length, Tm, doubles, wide, lambda v: np.array(v, dtype=wide).sum())
    c = [np.array(row, dtype=wide) for row in c]
    rr, cc = np.divmod(np.arange(P), Wm)
    S = sector[rr[:, None] - rr[None, :] + Hm - 1, cc[:, None] - cc[None, :] + Wm - 1].astype(np.int8)     # [b][a]: sector(b - a)
    one = wide(1)
    M = np.zeros((n + 1, n + 1), wide)
    A, total = one, wide(0)
    for t in range(Tm - 2):
        fin, fout = np.zeros((P, n + 1), wide), np.zeros((P, n + 1), wide)
        for k in range(n + 1):
            fin[:, k] = np.where(S == k, c[t][None, :], wide(0)).sum(1)
            fout[:, k] = np.where(S.T == k, c[t + 2][None, :], wide(0)).sum(1)
        M += A * ((c[t + 1][:, None] * fin).T @ fout)
        total += A * (one - q[t]) * (one - q[t + 1]) * (one - q[t + 2])
        A = A * (one - q[t])
    return M.astype(np.float64), float(total)


# ---- the host statistics, written independently (loops) ---------------------------------------------------------------------------------
def summary(table):
    table = np.asarray(table, dtype=np.float64)
    n = table.shape[0] - 1
    total = moving = sm = ms = 0.0
    turn = [0.0] * n
    for k in range(n + 1):
        for kk in range(n + 1):
            w = float(table[k, kk])
            total += w
            if k < n and kk < n:
                moving += w
                turn[(kk - k) % n] += w
            elif k == n and kk < n:
                sm += w
            elif k < n:
                ms += w
    hist = [v / moving if moving > 0 else NAN for v in turn]
    share = (lambda v: v / total) if total > 0 else (lambda v: NAN)
    return {"total": total, "moving": moving, "turn_hist": hist, "forward": hist[0], "reversal": hist[n // 2] if n % 2 == 0 else NAN,
            "persistence": sum(h * math.cos(2 * math.pi * m / n) for m, h in enumerate(hist)),
            "stay_then_move": share(sm), "move_then_stay": share(ms), "stay_then_stay": share(float(table[n, n])),
            "transition": [[float(table[k, kk]) / moving if moving > 0 else NAN for kk in range(n)] for k in range(n)]}
