"""Plain-loop float64 restatement of csrc/scansaccade.hip for the tests: sp_scan_saccade_counts and
sp_scan_saccade_expectation with the documented summation orders, written with Python floats (IEEE doubles, one rounding per operation)
and numpy float64 element-wise operations (one rounding each as well), and an independent copy of the host statistics written with
loops.  Nothing here imports the package."""
import math

import numpy as np

MAX_FIXATIONS = 64
MAX_CELLS = 2048
NAN = float("nan")


def cell(v, n, frame):
    """the pixel rule along one axis: floor(v * n / frame) in double"""
    return min(int(math.floor((v * float(n)) / frame)), n - 1)


def kept(x, y, fw, fh):
    return math.isfinite(x) and math.isfinite(y) and 0.0 <= x < fw and 0.0 <= y < fh


def saccade_counts(scanpaths, groups, n_groups, frame_size, map_shape, max_steps):
    """-> {"counts" int64 [G, 2 Hm - 1, 2 Wm - 1], "saccades" int32 [S], "dropped" int32 [S]}; a scanpath of more than MAX_FIXATIONS
    fixations or with a group outside [0, n_groups) is refused: saccades -1, dropped 0, nothing counted"""
    Hm, Wm = map_shape
    fh, fw = (float(v) for v in frame_size)
    S = len(scanpaths)
    counts = np.zeros((n_groups, 2 * Hm - 1, 2 * Wm - 1), np.int64)
    sacc, drop = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s, (sp, g) in enumerate(zip(scanpaths, groups)):
        sp = np.asarray(sp, dtype=np.float64)
        n = len(sp)
        if n > MAX_FIXATIONS or not 0 <= g < n_groups:
            sacc[s] = -1
            continue
        cells = []
        for i in range(min(n, max_steps)):
            x, y = float(sp[i, 0]), float(sp[i, 1])
            if kept(x, y, fw, fh):
                cells.append((cell(y, Hm, fh), cell(x, Wm, fw)))
            else:
                cells.append(None)
                drop[s] += 1
        for a, b in zip(cells[:-1], cells[1:]):
            if a is not None and b is not None:
                counts[g, b[0] - a[0] + Hm - 1, b[1] - a[1] + Wm - 1] += 1
                sacc[s] += 1
    return {"counts": counts, "saccades": sacc, "dropped": drop}


def lane_sum(values):
    """the kernel's order: lane l adds elements l, l + 64, .. from 0.0; the 64 partial sums combine by the xor butterfly 32 .. 1"""
    part = [0.0] * 64
    for i, v in enumerate(values):
        part[i % 64] = part[i % 64] + v
    for o in (32, 16, 8, 4, 2, 1):
        part = [part[l] + part[l ^ o] for l in range(64)]
    return part[0]


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def row_steps(p_row, min_length, Tm):
    """(c float64 [Tm, P], q [Tm]) of one row, or None for a bad row (a D_t, t < Tm, that is zero or not finite)"""
    wide = np.asarray(p_row, dtype=np.float32).astype(np.float64)          # exact
    cs, qs = [], []
    for t in range(Tm):
        Z = lane_sum(wide[t, 1:].tolist())
        stop = t >= min_length
        p0 = float(wide[t, 0]) if stop else 0.0
        D = Z + p0 if stop else Z
        if D == 0.0 or not math.isfinite(D):
            return None
        qs.append(_div(p0, D) if stop else 0.0)
        with np.errstate(all="ignore"):
            cs.append(wide[t, 1:] / np.float64(D))
    return np.array(cs).reshape(Tm, -1), qs


def cross_correlation(c0, c1, Hm, Wm):
    """X[d] = sum_i c0(i) c1(i + d) over the cells i whose partner lies inside the map, i in ascending row-major order from 0.0, every
    product rounded before it is added: looping over i and adding the window of products c0(i) * c1 to the lattice keeps that order for
    every d (each d receives at most one product per i)"""
    X = np.zeros((2 * Hm - 1, 2 * Wm - 1))
    grid = c1.reshape(Hm, Wm)
    for r in range(Hm):
        for c in range(Wm):
            # partner (r', c') gives dr = r' - r, dc = c' - c: lattice rows Hm - 1 - r .. 2 Hm - 2 - r, columns likewise
            X[Hm - 1 - r:2 * Hm - 1 - r, Wm - 1 - c:2 * Wm - 1 - c] += c0[r * Wm + c] * grid
    return X


def row_expectation(p_row, map_shape, min_length, max_steps):
    """(E_r float64 [2 Hm - 1, 2 Wm - 1], saccades, bad) of one row"""
    Hm, Wm = map_shape
    T = len(p_row)
    Tm = min(T, max_steps)
    E = np.zeros((2 * Hm - 1, 2 * Wm - 1))
    steps = row_steps(p_row, min_length, Tm)
    if steps is None:
        return E, NAN, 1
    c, q = steps
    A, total = 1.0, 0.0
    for t in range(Tm - 1):
        E = E + A * cross_correlation(c[t], c[t + 1], Hm, Wm)
        total = total + A * ((1.0 - q[t]) * (1.0 - q[t + 1]))
        A = A * (1.0 - q[t])
    return E, total, 0


def saccade_expectation(probs, row_groups, n_groups, map_shape, min_length, max_steps, rows=None):
    """probs float32 [R, T, 1 + P] -> {"E" float64 [G, 2 Hm - 1, 2 Wm - 1], "saccades" float64 [R], "bad" int32 [R], "rows": the
    per-row (E_r, saccades, bad), to be passed back as rows= with other groups}"""
    probs = np.asarray(probs, dtype=np.float32)
    R = probs.shape[0]
    Hm, Wm = map_shape
    assert probs.shape[2] == 1 + Hm * Wm and Hm * Wm <= MAX_CELLS
    E = np.zeros((n_groups, 2 * Hm - 1, 2 * Wm - 1))
    sacc, bad = np.full(R, NAN), np.zeros(R, np.int32)
    per_row = [None] * R if rows is None else rows
    for r in range(R):                                                   # ascending row index
        g = int(row_groups[r])
        if not 0 <= g < n_groups:
            bad[r] = -1
            continue
        if per_row[r] is None:
            per_row[r] = row_expectation(probs[r], map_shape, min_length, max_steps)
        Er, s, b = per_row[r]
        sacc[r], bad[r] = s, b
        if b == 0:
            E[g] = E[g] + Er
    return {"E": E, "saccades": sacc, "bad": bad, "rows": per_row}


def row_expectation_exact(p_row, map_shape, min_length, max_steps, doubles=False):
    """The closed form of a good row without any summation order: every float32 input is taken as the rational it is and Z, D, q, c, A,
    X and E are rationals (fractions.Fraction); only the results are rounded to double.  -> (E float64 [2 Hm - 1, 2 Wm - 1], saccades).
    doubles=True: c_t(i) and q_t are the DOUBLES of row_steps (the kernel's Z order and divisions), taken as the rationals they are --
    the exactly added exact products of what the kernel multiplies.  P * P * T rational products: for small maps only."""
    from fractions import Fraction
    Hm, Wm = map_shape
    P = Hm * Wm
    Tm = min(len(p_row), max_steps)
    c, q = [], []
    if doubles:
        cd, qd = row_steps(p_row, min_length, Tm)
        c, q = [[Fraction(float(v)) for v in row] for row in cd], [Fraction(float(v)) for v in qd]
    for t in range(0 if doubles else Tm):
        cells = [Fraction(float(v)) for v in p_row[t][1:]]
        stop = t >= min_length
        p0 = Fraction(float(p_row[t][0])) if stop else Fraction(0)
        D = sum(cells) + p0
        c.append([v / D for v in cells])
        q.append(p0 / D)
    E = [[Fraction(0)] * (2 * Wm - 1) for _ in range(2 * Hm - 1)]
    A, total = Fraction(1), Fraction(0)
    for t in range(Tm - 1):
        for i in range(P):
            if c[t][i]:
                w = A * c[t][i]
                for j in range(P):
                    E[j // Wm - i // Wm + Hm - 1][j % Wm - i % Wm + Wm - 1] += w * c[t + 1][j]
        total += A * (1 - q[t]) * (1 - q[t + 1])
        A *= 1 - q[t]
    return np.array([[float(v) for v in row] for row in E]), float(total)


def row_expectation_wide(p_row, map_shape, min_length, max_steps, doubles=False):
    """The same in numpy's extended precision (np.longdouble, 64 significant bits on x86: 2^-11 of a double's rounding per operation)
    and in another order (Z by numpy's pairwise sum, X by whole-window adds) -- for maps too large for rationals"""
    Hm, Wm = map_shape
    Tm = min(len(p_row), max_steps)
    wide = np.asarray(p_row, dtype=np.float32).astype(np.longdouble)
    one = np.longdouble(1)
    c, q = [], []
    if doubles:                                                          # the doubles the kernel multiplies (row_expectation_exact)
        cd, qd = row_steps(p_row, min_length, Tm)
        c, q = [row.astype(np.longdouble) for row in cd], [np.longdouble(v) for v in qd]
    for t in range(0 if doubles else Tm):
        stop = t >= min_length
        p0 = wide[t, 0] if stop else np.longdouble(0)
        D = wide[t, 1:].sum() + p0
        c.append(wide[t, 1:] / D)
        q.append(p0 / D)
    E = np.zeros((2 * Hm - 1, 2 * Wm - 1), np.longdouble)
    A, total = one, np.longdouble(0)
    for t in range(Tm - 1):
        grid = c[t + 1].reshape(Hm, Wm)
        for r in range(Hm):
            for k in range(Wm):
                E[Hm - 1 - r:2 * Hm - 1 - r, Wm - 1 - k:2 * Wm - 1 - k] += (A * c[t][r * Wm + k]) * grid
        total += A * (one - q[t]) * (one - q[t + 1])
        A = A * (one - q[t])
    return E.astype(np.float64), float(total)


# ---- the host statistics, written independently (loops, no bincount) ------------------------------------------------------------------
def vectors(map_shape, frame_size):
    Hm, Wm = map_shape
    fh, fw = (float(v) for v in frame_size)
    out = {}
    for dr in range(-(Hm - 1), Hm):
        for dc in range(-(Wm - 1), Wm):
            dx, dy = dc * fw / Wm, dr * fh / Hm
            out[(dr, dc)] = (dx, dy, math.sqrt(dx * dx + dy * dy))
    return out


def summary(lattice, frame_size, amplitude_edges, n_directions):
    lattice = np.asarray(lattice, dtype=np.float64)
    Hm, Wm = (lattice.shape[0] + 1) // 2, (lattice.shape[1] + 1) // 2
    edges, n = [float(e) for e in amplitude_edges], int(n_directions)
    total = moved = stay = amp_sum = over = 0.0
    hist, dirs = [0.0] * (len(edges) - 1), [0.0] * n
    for (dr, dc), (dx, dy, amp) in vectors((Hm, Wm), frame_size).items():
        w = float(lattice[dr + Hm - 1, dc + Wm - 1])
        total += w
        amp_sum += w * amp
        if amp >= edges[-1]:
            over += w
        for k in range(len(edges) - 1):
            if edges[k] <= amp < edges[k + 1]:
                hist[k] += w
        if dr == 0 and dc == 0:
            stay += w
        else:
            moved += w
            dirs[int(math.floor(math.atan2(dy, dx) * n / (2 * math.pi) + 0.5)) % n] += w
    if total <= 0:
        return {"total": total, "stay": NAN, "mean_amplitude": NAN, "amplitude_hist": [NAN] * len(hist), "amplitude_overflow": NAN,
                "direction_hist": [NAN] * n}
    return {"total": total, "stay": stay / total, "mean_amplitude": amp_sum / total, "amplitude_hist": [h / total for h in hist],
            "amplitude_overflow": over / total, "direction_hist": [d / moved if moved > 0 else NAN for d in dirs]}


def jensen_shannon(p, q):
    p, q = [float(v) for v in np.asarray(p).reshape(-1)], [float(v) for v in np.asarray(q).reshape(-1)]
    sp, sq = math.fsum(p), math.fsum(q)
    if not (sp > 0 and sq > 0 and math.isfinite(sp) and math.isfinite(sq)):
        return NAN
    total = 0.0
    for a, b in zip(p, q):
        a, b = a / sp, b / sq
        m = (a + b) / 2
        if a > 0:
            total += 0.5 * a * math.log2(a / m)
        if b > 0:
            total += 0.5 * b * math.log2(b / m)
    return total


def wasserstein_amplitude(lattice_a, lattice_b, frame_size):
    a, b = np.asarray(lattice_a, dtype=np.float64), np.asarray(lattice_b, dtype=np.float64)
    Hm, Wm = (a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2
    sa, sb = float(a.sum()), float(b.sum())
    if not (sa > 0 and sb > 0):
        return NAN
    mass = {}
    for (dr, dc), (_, _, amp) in vectors((Hm, Wm), frame_size).items():
        pa, pb = mass.get(amp, (0.0, 0.0))
        mass[amp] = (pa + float(a[dr + Hm - 1, dc + Wm - 1]) / sa, pb + float(b[dr + Hm - 1, dc + Wm - 1]) / sb)
    values = sorted(mass)
    ca = cb = total = 0.0
    for v, nxt in zip(values[:-1], values[1:]):
        ca, cb = ca + mass[v][0], cb + mass[v][1]
        total += abs(ca - cb) * (nxt - v)
    return total
