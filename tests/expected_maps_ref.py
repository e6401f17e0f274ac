"""Plain-loop float64 restatement of csrc/scanexpect.hip for the tests: sp_model_fixation_expectation with the
documented order of every sum, written with Python floats and numpy float64 element-wise operations (one rounding per operation), a
numpy float32 restatement of the cell-pixel table, and the exhaustive enumeration of all action sequences in exact rationals.  Z, D, q
and c are those of tests/saccade_statistics_ref.py (row_steps).  Nothing here imports the package.

THE ORDER OF EVERY SUM, restated: Z_t by lane_sum (lane l adds cells l, l + 64, .. from 0.0, then the xor butterfly 32 .. 1); A in
ascending t from 1.0, A_{t+1} = A_t * (1.0 - q_t); w_t = A_t * (1.0 - q_t); f_t = A_t * s_t (A_t without a weight); e_r(i) in
ascending t from 0.0, each term the rounded quotient c_t(i) times the rounded f_t; fixations in ascending t from 0.0; m_g(i) in
ascending row index from 0.0; maps[g][px] in ascending cell index from 0.0; a pixel without a cell is 0.0, an empty group a zero map."""
import itertools
import math
from fractions import Fraction

import numpy as np

from saccade_statistics_ref import MAX_CELLS, MAX_FIXATIONS, NAN, row_steps  # noqa: F401

U = 2.0 ** -53


def cell_pixels(map_shape, frame_size, output_shape=None):
    """int32 [Hm Wm]: the sampler's pixel of every cell in its float32 arithmetic -- xg = (float)width / (float)map_w, x = c * xg +
    0.5f * xg with ONE rounding (the product and the sum are exact in float64 up to its own last bit, then rounded to float32), rows
    likewise -- pushed through THE PIXEL RULE min(floor(v * n / frame), n - 1) in float64"""
    Hm, Wm = map_shape
    fh, fw = (int(v) for v in frame_size)
    H, W = (fh, fw) if output_shape is None else (int(v) for v in output_shape)

    def axis(ncell, frame, n):
        g = np.float32(frame) / np.float32(ncell)
        v = (np.arange(ncell, dtype=np.float64) * np.float64(g) + np.float64(np.float32(0.5) * g)).astype(np.float32).astype(np.float64)
        assert (v >= 0).all() and (v < frame).all()
        return np.minimum(np.floor(v * n / float(frame)), n - 1).astype(np.int64)

    row, col = axis(Hm, fh, H), axis(Wm, fw, W)
    return (row[:, None] * W + col[None, :]).reshape(-1).astype(np.int32)


def row_map(p_row, weight_row, min_length, max_steps):
    """(e_r float64 [P], fixations, bad) of one row; weight_row None or [T]"""
    p_row = np.asarray(p_row, dtype=np.float32)
    T, P = p_row.shape[0], p_row.shape[1] - 1
    Tm = min(T, max_steps)
    e = np.zeros(P)
    if weight_row is not None and any(not math.isfinite(float(s)) or float(s) < 0.0 for s in weight_row[:Tm]):
        return e, NAN, 1
    steps = row_steps(p_row, min_length, Tm)
    if steps is None:
        return e, NAN, 1
    c, q = steps
    A, fix = 1.0, 0.0
    for t in range(Tm):
        w = A * (1.0 - q[t])
        f = A if weight_row is None else A * float(weight_row[t])
        e = e + c[t] * np.float64(f)
        fix = fix + w
        A = A * (1.0 - q[t])
    return e, fix, 0


def expected_fixation_maps(probs, step_weight, row_groups, n_groups, min_length, max_steps, cell_pixel, H, W, rows=None):
    """probs float32 [R, T, 1 + P] -> {"maps" float64 [G, H, W], "fixations" float64 [R], "bad" int32 [R], "rows": the per-row (e_r,
    fixations, bad), to be passed back as rows= with other groups or another cell_pixel}"""
    probs = np.asarray(probs, dtype=np.float32)
    R, P = probs.shape[0], probs.shape[2] - 1
    assert P == len(cell_pixel) <= MAX_CELLS and 1 <= max_steps <= MAX_FIXATIONS
    m = np.zeros((n_groups, P))
    fixations, bad = np.full(R, NAN), np.zeros(R, np.int32)
    per_row = [None] * R if rows is None else rows
    for r in range(R):                                                   # ascending row index
        g = int(row_groups[r])
        if not 0 <= g < n_groups:
            bad[r] = -1
            continue
        if per_row[r] is None:
            per_row[r] = row_map(probs[r], None if step_weight is None else step_weight[r], min_length, max_steps)
        e, fix, b = per_row[r]
        fixations[r], bad[r] = fix, b
        if b == 0:
            m[g] = m[g] + e
    maps = np.zeros((n_groups, H * W))
    for i in range(P):                                                   # ascending cell index
        px = int(cell_pixel[i])
        if 0 <= px < H * W:
            maps[:, px] = maps[:, px] + m[:, i]
    return {"maps": maps.reshape(n_groups, H, W), "fixations": fixations, "bad": bad, "rows": per_row}


def step_distributions(p_row, min_length):
    """the sampler's rule in exact rationals: per step the probability of every action, terminate (action 0) masked for t < min_length"""
    exact = [[Fraction(float(v)) for v in step] for step in np.asarray(p_row, dtype=np.float32)]
    out = []
    for t, step in enumerate(exact):
        allowed = range(1, len(step)) if t < min_length else range(len(step))
        total = sum(step[k] for k in allowed)
        out.append([step[a] / total if a in allowed else Fraction(0) for a in range(len(step))])
    return out


def enumerate_sequences(p_row, min_length):
    """every action sequence of non-zero probability with that probability (exact; they add up to 1)"""
    step = step_distributions(p_row, min_length)
    for seq in itertools.product(range(len(step[0])), repeat=len(step)):
        w = Fraction(1)
        for t, a in enumerate(seq):
            w *= step[t][a]
            if not w:
                break
        if w:
            yield seq, w


def enumerated_map(p_row, weight_row, min_length, max_steps, cell_pixel, HW):
    """(the expected map as HW exact rationals, the expected number of fixations): all (1 + P)^T sequences; the first terminate ends the
    scanpath, only the first max_steps fixations count, fixation t weighs weight_row[t] (1 without weights)"""
    want, fixations, mass = [Fraction(0)] * HW, Fraction(0), Fraction(0)
    for seq, w in enumerate_sequences(p_row, min_length):
        mass += w
        for t, a in enumerate(list(itertools.takewhile(lambda a: a != 0, seq))[:max_steps]):
            want[int(cell_pixel[a - 1])] += w * (1 if weight_row is None else Fraction(float(weight_row[t])))
            fixations += w
    assert mass == 1
    return want, fixations


def roundings(P, T, cells_per_pixel, conditioning):
    """an upper count of the roundings behind one entry of the restatement's map of ONE row, for the relative bound roundings * 2^-53
    (all terms are non-negative, so relative errors add and never amplify -- except in 1.0 - q_t, where the relative error of q_t is
    multiplied by q_t / (1 - q_t) = p_0 / Z <= conditioning, a property of the test's inputs that the test states and asserts):
      Z_t: at most P additions;  D_t: 1;  q_t: 1  -> P + 2;   1 - q_t: conditioning * (P + 2) + 1 =: k;
      A_t = the product of t such factors with t multiplications, w_t one more of each: at most T (k + 1);   f_t: 1;   c_t(i): P + 1 for D_t and 1;
      a term c_t(i) * f_t: 1;   the sum over t: T;   the sum over a pixel's cells: cells_per_pixel;   the conversion of the exact
      value to float64 on the other side: 1"""
    k = conditioning * (P + 2) + 1
    return T * (k + 1) + 1 + (P + 2) + 1 + T + cells_per_pixel + 1


def bound(P, T, cells_per_pixel, conditioning):
    """the relative bound of a comparison against the enumeration: gamma_n = n u / (1 - n u), u = 2^-53, with n = the (1 + P)^T terms
    the enumeration adds into one entry (as DESIGN.md §25 counts them) + roundings(..)"""
    n = (1 + P) ** T + roundings(P, T, cells_per_pixel, conditioning)
    return n * U / (1.0 - n * U)
