"""Recurrence statistics on the device (csrc/scanrecur.hip in libscanpaths_amd_stats.so): how often a scanpath comes
back to a place it has already looked at, and after how many fixations -- the upper-triangle auto-recurrence form of Anderson et al.
2013 on action-map cells, read by lag as the direct measure of inhibition of return (Klein 2000) -- for scanpaths that
exist and, in closed form, for the model's own step distributions:

    res = recurrence_counts(scanpaths, groups, n_groups, frame_size, map_shape, max_steps=16, radius=16.0, min_line=2)    # humans, samples
    # {"counts": int64 [G, K, K], "points": int32 [S], "dropped": int32 [S], "rqa": int32 [S, 6]}, K = max_steps
    res = recurrence_expectation(probs, row_groups, n_groups, min_length=1, max_steps=16, radius=16.0, frame_size=(240, 320))
    # {"E": float64 [G, K, K], "points": float64 [R], "bad": int32 [R]}
    s = recurrence_summary(res["E"][0])

One rule for humans, samples and the model.  Fixations are cells (the pixel rule of saccade_statistics), and two fixations are
RECURRENT iff the pixel length of their cell displacement is at most radius: recurrence_mask decides that once, on the host, in
float64, and both kernels only read the table, so a displacement on the boundary cannot land differently on the two sides of a
comparison.  The table [K, K], K = max_steps <= 64, is read as a recurrence plot: for s < t entry [s, t] (upper triangle) counts the
recurrent pairs (fixation s, fixation t), entry [t, s] (lower triangle) the pairs that exist at all -- the denominator -- and entry
[t, t] the fixations t.
recurrence_counts: only the first min(n_fix, max_steps) fixations of a scanpath count; a fixation outside the frame or with a non-finite
coordinate is dropped ("dropped"): it recurs with nothing, is in no pair and breaks every line through it.  "points" = the recurrent
pairs per scanpath; "rqa" [S, 6] = the integers of Anderson et al. 2013 on the upper triangle, main diagonal excluded: N (kept
fixations), R (recurrent points), the points on diagonal ((i, j), (i + 1, j + 1), ..), horizontal (fixed i, consecutive j) and vertical
(fixed j, consecutive i) lines of at least min_line points, and sum (j - i) over the recurrent points, all in original ordinals (a
dropped fixation is not compacted away).  recurrence_measures turns them into REC, DET, LAM and CORM.  Integers, hence exact.
recurrence_expectation: probs [R, T, 1 + P] are the model's eval-mode step distributions.  The decoder is not conditioned on sampled
fixations, so given the image fixations s and t of a sample are independent, and the sample reaches fixation t iff no terminate was
drawn up to t: with Z, D, q, c, A of saccade_expectation (the same summation order: bad rows agree) and Tm = min(T, max_steps),
    G_st = prod_{s<u<t} (1 - q_u),  B_t(i) = sum of c_t over the cells within the mask of cell i,  X_st = sum_i c_s(i) B_t(i)
    E[s, t] = (A_s G_st) X_st,  E[t, s] = (A_s G_st) ((1 - q_s) (1 - q_t)),  E[t, t] = A_t (1 - q_t),  points[r] = sum_{s<t} E_r[s, t]
and E[g] adds the E_r of the good rows of group g in ascending row index: exact, no sampling noise (the order of every sum:
csrc/scanrecur.hip).  Bad rows ("bad" 1, "points" NaN, nothing added) as in saccade_expectation.  The cost of a call grows with the
number of 1-entries of the mask (every cell of every step map adds up the cells within the radius); no run-length or prefix-sum
shortcut is taken.  DET and LAM of the model are line statistics without a pairwise closed form: they come from samples through
recurrence_counts.  max_steps at most 64, maps of at most 2048 cells; max_steps, min_length, radius, min_line and frame_size have no
defaults.  R Tm^2 + (2 Hm - 1)(2 Wm - 1) / 2 + 1 doubles of device scratch per call; probs stays on the device.  There is no CPU path.
recurrence_measures, recurrence_summary and recurrence_comparison are pure numpy; the last two take integer counts or expectations."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ... import hip
from . import _batch
from ._args import MAX_CELLS, check_frame, check_map, check_map_shape, check_min_length, check_probs, check_steps
from ._batch import MAX_FIXATIONS
from ._grouped import grouped_counts, grouped_expectation
from .saccade_statistics import jensen_shannon, lattice_vectors

RQA = ("N", "R", "diagonal", "horizontal", "vertical", "lag_sum")     # the columns of "rqa"


def _device() -> torch.device:
    return _batch.device("recurrence statistics run")


def _library():
    """libscanpaths_amd_stats.so, its limits held to this side's, or HipError"""
    L = hip.stats_lib()
    if L.sp_stats_max_fixations() != MAX_FIXATIONS or L.sp_stats_max_cells() != MAX_CELLS:
        raise hip.HipError(f"kernel limits {L.sp_stats_max_fixations()} / {L.sp_stats_max_cells()}, this module expects "
                           f"{MAX_FIXATIONS} / {MAX_CELLS}")
    return L


def check_table_steps(max_steps) -> int:
    """max_steps, the side of the table: an integer in [1, 64]"""
    max_steps = check_steps(max_steps)
    if max_steps > MAX_FIXATIONS:
        raise ValueError(f"max_steps {max_steps}: a recurrence table has at most {MAX_FIXATIONS} steps a side")
    return max_steps


def check_radius(radius) -> float:
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not np.isfinite(radius) or radius < 0:
        raise ValueError(f"radius {radius!r}: a finite number of pixels >= 0")
    return float(radius)


def check_min_line(min_line) -> int:
    if min_line is None or isinstance(min_line, bool) or int(min_line) != min_line or int(min_line) < 2:
        raise ValueError(f"min_line {min_line!r}: an integer >= 2")
    return int(min_line)


def check_table(table) -> np.ndarray:
    a = np.asarray(table)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"a recurrence table is a [max_steps, max_steps] array, got shape {a.shape}")
    return a.astype(np.float64)


def recurrence_mask(map_shape, frame_size, radius) -> np.ndarray:
    """uint8 [2 Hm - 1, 2 Wm - 1]: entry [dr + Hm - 1, dc + Wm - 1] is 1 iff sqrt(dx * dx + dy * dy) <= radius in float64, dx and dy
    the pixel displacement of lattice_vectors -- the table both kernels read.  radius 0: only the same cell is recurrent."""
    radius = check_radius(radius)
    _, _, amplitude = lattice_vectors(map_shape, frame_size)
    return np.ascontiguousarray(amplitude <= radius, dtype=np.uint8)


# ---- device calls -------------------------------------------------------------------------------------------------------------------------
def recurrence_counts(scanpaths, groups, n_groups, frame_size, map_shape, *, max_steps, radius, min_line) -> Dict[str, np.ndarray]:
    """scanpaths: S arrays [n <= 64, >= 2] of (x, y, ...) or structured fixation vectors; groups [S] in [0, n_groups): the table each
    scanpath is counted into (an empty group stays zero); frame_size = (height, width); map_shape = (Hm, Wm), at most 2048 cells;
    max_steps <= 64; radius in pixels, finite and >= 0; min_line >= 2 (all three required).
    Returns {"counts": int64 [n_groups, max_steps, max_steps], "points": int32 [S], "dropped": int32 [S], "rqa": int32 [S, 6]} (module
    docstring)."""
    max_steps, radius, min_line = check_table_steps(max_steps), check_radius(radius), check_min_line(min_line)
    shape, frame = check_map_shape(map_shape), check_frame(frame_size)
    return grouped_counts("sp_stats_recurrence_counts", _device, scanpaths, groups, n_groups, frame, shape, max_steps,
                          shape=(max_steps, max_steps), unit="points", tables=lambda: {"mask": recurrence_mask(shape, frame, radius)},
                          scalars=(min_line,), library=_library, per_scanpath={"rqa": len(RQA)})


def recurrence_expectation(probs, row_groups, n_groups, *, min_length, max_steps, radius, frame_size, map_shape=None) -> Dict[str, np.ndarray]:
    """probs: device tensor [R, T, 1 + P] (any float dtype; detached and read as float32); row_groups [R] in [0, n_groups): the table
    each row is added into, in ascending row index; min_length: the sampler's; max_steps <= 64: only the first max_steps steps count;
    radius in pixels and frame_size = (height, width) give the mask (all four required); map_shape = (Hm, Wm) defaults to (30, 40) for
    1201 actions only.  The cost grows with the number of 1-entries of the mask.
    Returns {"E": float64 [n_groups, max_steps, max_steps], "points": float64 [R], "bad": int32 [R]} (module docstring)."""
    min_length, max_steps, radius = check_min_length(min_length), check_table_steps(max_steps), check_radius(radius)
    frame = check_frame(frame_size)
    R, T, A = check_probs(probs)
    shape = check_map(A, map_shape, max_cells=MAX_CELLS)
    Tm, D = min(T, max_steps), (2 * shape[0] - 1) * (2 * shape[1] - 1)
    return grouped_expectation("sp_stats_recurrence_expectation", _device, probs, shape, row_groups, n_groups, min_length, max_steps,
                               shape=(max_steps, max_steps), work=R * Tm * Tm + D // 2 + 1, name="E", unit="points",
                               tables=lambda: {"mask": recurrence_mask(shape, frame, radius)}, library=_library)


# ---- pure numpy ---------------------------------------------------------------------------------------------------------------------------
def recurrence_measures(rqa) -> Dict[str, np.ndarray]:
    """rqa: the integers [S, 6] of recurrence_counts (or one row [6]) -> {"REC", "DET", "LAM", "CORM"}, float64 [S] each (Anderson et
    al. 2013): REC = 100 * 2 R / (N (N - 1)), DET = 100 * diagonal / R, LAM = 100 * (horizontal + vertical) / (2 R),
    CORM = 100 * lag_sum / ((N - 1) R); NaN where a denominator is 0 (N < 2 or R = 0)"""
    a = np.asarray(rqa)
    if a.ndim not in (1, 2) or a.shape[-1] != len(RQA) or (a.size and a.min() < 0):
        raise ValueError(f"rqa: non-negative integers of shape [S, {len(RQA)}] are required, got shape {a.shape}")
    N, R, DL, HL, VL, lag = (a.reshape(-1, len(RQA))[:, k].astype(np.float64) for k in range(len(RQA)))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"REC": np.where(N >= 2, 100.0 * (2.0 * R) / (N * (N - 1.0)), np.nan),
               "DET": np.where(R > 0, 100.0 * DL / R, np.nan),
               "LAM": np.where(R > 0, 100.0 * (HL + VL) / (2.0 * R), np.nan),
               "CORM": np.where((R > 0) & (N >= 2), 100.0 * lag / ((N - 1.0) * R), np.nan)}
    return out


def _by_lag(a: np.ndarray):
    """(the upper and the lower triangle's sums per lag 1 .. K - 1)"""
    K = a.shape[0]
    return (np.array([np.trace(a, offset=k) for k in range(1, K)], dtype=np.float64),
            np.array([np.trace(a, offset=-k) for k in range(1, K)], dtype=np.float64))


def recurrence_summary(table) -> dict:
    """The descriptive statistics of one table [K, K] (integer counts or expectations):
      "fixations": the diagonal's sum;  "pairs": the lower triangle's sum;  "points": the upper triangle's sum;
      "REC" = 100 * points / pairs;  "recurrence_by_lag" float64 [K - 1]: for lag l = 1 .. K - 1 the share sum_s table[s, s + l] /
      sum_s table[s + l, s] of the pairs l fixations apart that are recurrent, NaN where there are no such pairs;
      "mean_lag" = sum (t - s) table[s, t] / points;  "mean_lag_chance": the same over the lower triangle -- the value of mean_lag when
      recurrence does not depend on the lag.
    Ratios without a denominator are NaN."""
    a = check_table(table)
    K = a.shape[0]
    upper, lower = _by_lag(a)
    points, pairs = float(upper.sum()), float(lower.sum())
    lags = np.arange(1, K, dtype=np.float64)
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"fixations": float(np.trace(a)), "pairs": pairs, "points": points, "REC": 100.0 * points / pairs if pairs > 0 else nan,
                "recurrence_by_lag": np.where(lower > 0, upper / lower, np.nan),
                "mean_lag": float((lags * upper).sum()) / points if points > 0 else nan,
                "mean_lag_chance": float((lags * lower).sum()) / pairs if pairs > 0 else nan}


def recurrence_comparison(table, human_table) -> dict:
    """A table against the human one: "REC_difference" = REC - the human REC (percentage points); "L1_by_lag": the mean absolute
    difference of "recurrence_by_lag" over the lags defined on both sides (NaN without one); "JSD_lag": jensen_shannon, in bits, of the
    two lag profiles sum_s table[s, s + l] -- where along the lag axis the recurrent points sit"""
    a, h = check_table(table), check_table(human_table)
    if a.shape != h.shape:
        raise ValueError(f"tables of shapes {a.shape} and {h.shape}: one shape is required")
    mine, theirs = recurrence_summary(a), recurrence_summary(h)
    both = ~np.isnan(mine["recurrence_by_lag"]) & ~np.isnan(theirs["recurrence_by_lag"])
    gap = np.abs(mine["recurrence_by_lag"][both] - theirs["recurrence_by_lag"][both])
    return {"REC_difference": mine["REC"] - theirs["REC"], "L1_by_lag": float(gap.mean()) if both.any() else float("nan"),
            "JSD_lag": jensen_shannon(_by_lag(a)[0], _by_lag(h)[0])}
