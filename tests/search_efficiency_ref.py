"""Plain-loop float64 restatement of csrc/scansearch.hip for the tests: sp_scan_target_hits and sp_scan_target_mass with
the documented summation orders and the sampler's float32 pixel, written with Python floats (IEEE doubles, one rounding per operation)
and np.float32 scalars.  Nothing here imports the package."""
import math

import numpy as np

MAX_FIXATIONS = 64
MAX_SIDE = 1024
NAN = float("nan")


def dist(dx, dy):
    """scan_dist: three roundings and the correctly rounded root"""
    return math.sqrt(dx * dx + dy * dy)


def inside(x, y, box):
    x0, y0, x1, y1 = (float(v) for v in box)
    return math.isfinite(x) and math.isfinite(y) and x0 <= x < x1 and y0 <= y < y1


def target_hits(scanpaths, boxes, max_steps):
    """-> {"hit" int32 [S], "path", "SPR" float64 [S], "n" int32 [S]}"""
    S = len(scanpaths)
    hit, path, spr, cnt = np.full(S, -1, np.int32), np.full(S, NAN), np.full(S, NAN), np.zeros(S, np.int32)
    for s, (sp, box) in enumerate(zip(scanpaths, boxes)):
        sp = np.asarray(sp, dtype=np.float64)
        sp = sp.reshape(len(sp), -1) if sp.size else np.zeros((0, 2))
        n = len(sp)
        cnt[s] = min(n, max_steps)
        if n > MAX_FIXATIONS:
            continue
        xy = [(float(sp[i, 0]), float(sp[i, 1])) for i in range(min(n, max_steps))]
        h = next((i for i, (x, y) in enumerate(xy) if inside(x, y, box)), -1)
        hit[s] = h
        if h < 0:
            continue
        total = 0.0
        for i in range(1, h + 1):                                      # left to right in index order
            total = total + dist(xy[i][0] - xy[i - 1][0], xy[i][1] - xy[i - 1][1])
        x0, y0, x1, y1 = (float(v) for v in box)
        ratio = 1.0 if h == 0 else _div(dist(xy[0][0] - (x0 + x1) / 2.0, xy[0][1] - (y0 + y1) / 2.0), total)
        if any(not (math.isfinite(x) and math.isfinite(y)) for x, y in xy[:h]):
            total = ratio = NAN
        path[s], spr[s] = total, ratio
    return {"hit": hit, "path": path, "SPR": spr, "n": cnt}


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def centres(n, frame, fused=True):
    """the sampler's pixel of index 0 .. n - 1 along a side of `frame` pixels, float32 arithmetic through np.float32, widened to double:
    g = (float)(frame / n), half = 0.5f * g, pixel = fmaf((float)k, g, half) -- ONE rounding, which is what csrc/sampling.hip's
    `(float)k * g + 0.5f * g` compiles to under the default contraction.  The fused value is restated as the float32 rounding of the
    float64 expression k * g + half, which is exact: k < 2^10 and g has 24 significant bits, so the product has at most 34 and the sum
    with half (one binade below g) at most 36.  fused=False rounds the product on its own: the source text read literally, kept to show
    where the two differ (row 6 of 7 on 75 pixels)."""
    with np.errstate(all="ignore"):
        g = np.float32(float(frame) / n)
        half = np.float32(0.5) * g
        if fused:
            return [float(np.float32(float(k) * float(g) + float(half))) for k in range(n)]
        return [float(np.float32(np.float32(k) * g) + half) for k in range(n)]


def cell_range(n, frame, lo, hi):
    """[first, end) of the members lo <= centre < hi of one axis, (0, 0) without one"""
    lo, hi = float(lo), float(hi)
    mem = [k for k, c in enumerate(centres(n, frame)) if lo <= c < hi]
    return (mem[0], mem[-1] + 1) if mem else (0, 0)


def lane_sum(values):
    """the kernel's order: lane l adds elements l, l + 64, .. from 0.0; the 64 partial sums combine by the xor butterfly 32 .. 1"""
    part = [0.0] * 64
    for i, v in enumerate(values):
        part[i % 64] = part[i % 64] + v
    for o in (32, 16, 8, 4, 2, 1):
        part = [part[l] + part[l ^ o] for l in range(64)]
    return part[0]


def step_sums(probs, boxes, box_rows, frame_size, map_shape):
    """what does not depend on min_length: (Z float64 [R, T], B float64 [NB, T], cells int32 [NB]) in the kernel's summation orders;
    cells -1 (and nothing summed) for a box whose row does not exist"""
    probs = np.asarray(probs, dtype=np.float32)
    R, T, A = probs.shape
    Hm, Wm = map_shape
    fh, fw = frame_size
    assert A == 1 + Hm * Wm and 1 <= Hm <= MAX_SIDE and 1 <= Wm <= MAX_SIDE
    NB = len(boxes)
    wide = probs.astype(np.float64)                                     # exact
    Z = np.full((R, T), NAN)
    for row in sorted({int(r) for r in box_rows if 0 <= r < R}):
        for t in range(T):
            Z[row, t] = lane_sum(wide[row, t, 1:].tolist())
    B, cells = np.full((NB, T), NAN), np.zeros(NB, np.int32)
    for b, (box, row) in enumerate(zip(boxes, box_rows)):
        if not 0 <= row < R:
            cells[b] = -1
            continue
        c0, c1 = cell_range(Wm, fw, box[0], box[2])
        r0, r1 = cell_range(Hm, fh, box[1], box[3])
        cells[b] = (r1 - r0) * (c1 - c0)
        for t in range(T):
            grid = wide[row, t, 1:].reshape(Hm, Wm)
            B[b, t] = lane_sum(grid[r0:r1, c0:c1].reshape(-1).tolist() if cells[b] else [])     # row-major order of the rectangle
    return Z, B, cells


def target_mass(probs, boxes, box_rows, frame_size, map_shape, min_length, sums=None):
    """probs float32 [R, T, 1 + P]; boxes [NB, 4]; frame_size = (height, width) -> {"MASS", "HIT", "TFP" float64 [NB, T], "cells" int32};
    sums: step_sums of the same arguments, to share them between several min_length"""
    probs = np.asarray(probs, dtype=np.float32)
    T = probs.shape[1]
    Z, B, cells = step_sums(probs, boxes, box_rows, frame_size, map_shape) if sums is None else sums
    NB = len(boxes)
    MASS, HIT, TFP = (np.full((NB, T), NAN) for _ in range(3))
    for b, row in enumerate(box_rows):
        if cells[b] < 0:
            continue
        A_t, tfp = 1.0, 0.0
        for t in range(T):
            stop = t >= min_length
            p0 = float(probs[row, t, 0]) if stop else 0.0
            D = float(Z[row, t]) + p0 if stop else float(Z[row, t])
            m = _div(float(B[b, t]), D)
            q = _div(p0, D) if stop else 0.0
            if D == 0.0 or D != D or m != m or q != q:
                break                                                   # NaN from here on
            MASS[b, t] = m
            HIT[b, t] = A_t * m
            tfp = tfp + HIT[b, t]
            TFP[b, t] = tfp
            A_t = A_t * ((1.0 - q) - m)
    return {"MASS": MASS, "HIT": HIT, "TFP": TFP, "cells": cells.copy()}


def search_curve(hit, max_steps):
    hit = np.asarray(hit)
    return np.array([np.mean((hit >= 0) & (hit <= k)) if len(hit) else NAN for k in range(max_steps)], dtype=np.float64)
