"""Turning angles on the device (csrc/scanturn.hip): how the direction of a saccade depends on the direction of the
saccade before it -- the direction-transition table and the turning-angle histogram with its forward peak and its return peak at 180
degrees, the signature of inhibition of return (Tatler & Vincent 2009; Le Meur & Liu 2015; Kuemmerer & Bethge 2021) -- for
scanpaths that exist and, in closed form, for the model's own step distributions:

    res = turn_counts(scanpaths, groups, n_groups, frame_size, map_shape, max_steps=16, n_directions=8)         # humans, samples
    # {"counts": int64 [G, n + 1, n + 1], "pairs": int32 [S], "dropped": int32 [S]}
    res = turn_expectation(probs, row_groups, n_groups, min_length=1, max_steps=16, frame_size=(240, 320), n_directions=8)
    # {"M": float64 [G, n + 1, n + 1], "pairs": float64 [R], "bad": int32 [R]}
    s = turn_summary(res["M"][0])

One rule for humans, samples and the model.  Fixations are cells and saccades cell displacements on the lattice of
saccade_statistics; turn_sectors gives every displacement ONE direction sector -- direction_sectors' float64 rule, with the zero
displacement as sector n, "stayed in the cell" -- and that table is built here, on the host, uploaded and only read by both kernels, so
a vector on a sector boundary cannot land differently on the two sides of a comparison.  The transition table M [n + 1, n + 1]:
M[k, k'] = the number of consecutive saccade pairs (fixation t -> t + 1, then t + 1 -> t + 2) whose first saccade is in sector k and
whose second is in sector k'; row and column n hold the stays; its mass is the number of pairs.
turn_counts: only the first min(n_fix, max_steps) fixations of a scanpath count; a fixation outside the frame or with a non-finite
coordinate is dropped ("dropped"), and pair t counts iff fixations t, t + 1 and t + 2 are all kept -- nothing bridges a dropped
fixation, so one dropped in the middle removes three pairs.  "pairs" = the number counted per scanpath.  Integers, hence exact.
turn_expectation: probs [R, T, 1 + P] are the model's eval-mode step distributions.  The decoder is not conditioned on sampled
fixations, so given the middle fixation b the incoming and the outgoing saccade are independent and the expected count factorises per
middle cell: with Z, D, q, c, A of saccade_expectation (the same summation order: bad rows agree) and Tm = min(T, max_steps),
    in_t[b][k] = sum_a c_t(a) [sector(b - a) = k],  out_t[b][k'] = sum_a c_{t+2}(a) [sector(a - b) = k']        (ascending row-major a)
    X_t[k][k'] = sum_b (c_{t+1}(b) * in_t[b][k]) * out_t[b][k']                                                 (ascending b)
    M_r = sum_{t=0}^{Tm-3} A_t * X_t,  pairs[r] = sum_t A_t * (((1 - q_t) * (1 - q_{t+1})) * (1 - q_{t+2}))        (ascending t)
and M[g] adds the M_r of the good rows of group g in ascending row index: exact, no sampling noise.  Bad rows ("bad" 1, "pairs" NaN,
nothing added) as in saccade_expectation; Tm < 3: no pair.  n_directions at most 16 (the kernel's bins live in LDS), maps of at most
2048 cells; n_directions, max_steps, min_length and frame_size have no defaults.  R max(Tm - 2, 1) (n + 1)^2 doubles of device scratch
per call; probs stays on the device.  There is no CPU path.
turn_summary and turn_comparison are pure numpy and take integer counts or expectations alike."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _batch
from ._args import MAX_CELLS, MAX_DIRECTIONS, check_directions, check_frame, check_map, check_map_shape, check_min_length, check_probs, check_steps
from ._batch import MAX_FIXATIONS  # noqa: F401  (re-exported)
from ._grouped import grouped_counts, grouped_expectation
from .saccade_statistics import direction_sectors, jensen_shannon


def _device() -> torch.device:
    return _batch.device("turn statistics run")


def check_table(table) -> np.ndarray:
    a = np.asarray(table)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 2:
        raise ValueError(f"a transition table is an [n + 1, n + 1] array with n >= 1, got shape {a.shape}")
    return a.astype(np.float64)


def turn_sectors(map_shape, frame_size, n_directions) -> np.ndarray:
    """int32 [2 Hm - 1, 2 Wm - 1]: direction_sectors(map_shape, frame_size, n_directions) with the zero displacement as sector
    n_directions ("stayed in the cell") instead of -1 -- the table both kernels read"""
    n = check_directions(n_directions, MAX_DIRECTIONS)
    k = direction_sectors(map_shape, frame_size, n)
    k[k < 0] = n
    return np.ascontiguousarray(k, dtype=np.int32)


# ---- device calls -------------------------------------------------------------------------------------------------------------------------
def turn_counts(scanpaths, groups, n_groups, frame_size, map_shape, *, max_steps, n_directions) -> Dict[str, np.ndarray]:
    """scanpaths: S arrays [n <= 64, >= 2] of (x, y, ...) or structured fixation vectors; groups [S] in [0, n_groups): the table each
    scanpath is counted into (an empty group stays zero); frame_size = (height, width); map_shape = (Hm, Wm), at most 2048 cells.
    Returns {"counts": int64 [n_groups, n + 1, n + 1], "pairs": int32 [S], "dropped": int32 [S]} (module docstring)."""
    max_steps, n = check_steps(max_steps), check_directions(n_directions, MAX_DIRECTIONS)
    shape, frame = check_map_shape(map_shape), check_frame(frame_size)
    return grouped_counts("sp_scan_turn_counts", _device, scanpaths, groups, n_groups, frame, shape, max_steps, shape=(n + 1, n + 1),
                          unit="pairs", tables=lambda: {"sector": turn_sectors(shape, frame, n)}, scalars=(n,))


def turn_expectation(probs, row_groups, n_groups, *, min_length, max_steps, frame_size, n_directions, map_shape=None) -> Dict[str, np.ndarray]:
    """probs: device tensor [R, T, 1 + P] (any float dtype; detached and read as float32); row_groups [R] in [0, n_groups): the table
    each row is added into, in ascending row index; min_length: the sampler's; max_steps: only the first max_steps steps count;
    frame_size = (height, width): the sectors are directions in pixels; n_directions <= 16 (all four required); map_shape = (Hm, Wm)
    defaults to (30, 40) for 1201 actions only.
    Returns {"M": float64 [n_groups, n + 1, n + 1], "pairs": float64 [R], "bad": int32 [R]} (module docstring)."""
    min_length, max_steps, n = check_min_length(min_length), check_steps(max_steps), check_directions(n_directions, MAX_DIRECTIONS)
    frame = check_frame(frame_size)
    R, T, A = check_probs(probs)
    shape = check_map(A, map_shape, max_cells=MAX_CELLS)
    return grouped_expectation("sp_scan_turn_expectation", _device, probs, shape, row_groups, n_groups, min_length, max_steps,
                               shape=(n + 1, n + 1), work=R * max(min(T, max_steps) - 2, 1) * (n + 1) * (n + 1), name="M", unit="pairs",
                               tables=lambda: {"sector": turn_sectors(shape, frame, n)}, scalars=(n,))


# ---- pure numpy, on one transition table ---------------------------------------------------------------------------------------------------
def turn_summary(table) -> dict:
    """The descriptive statistics of one transition table [n + 1, n + 1] (integer counts or expectations; n is read off its shape):
      "total": the table's mass (the number of saccade pairs);  "moving": the mass of table[:n, :n], the pairs of two real saccades;
      "turn_hist" float64 [n]: the share, among the moving pairs, of every turn m = (k' - k) mod n -- m sectors of 2 pi / n towards
      larger angles;  "forward" = turn_hist[0];  "reversal" = turn_hist[n / 2] for even n, NaN for odd n (no sector is opposite);
      "persistence" = sum_m turn_hist[m] cos(2 pi m / n): 1 for all forward, -1 for all reversal;  "stay_then_move", "move_then_stay",
      "stay_then_stay": the shares of total of table[n, :n], table[:n, n] and table[n, n];  "transition" float64 [n, n] =
      table[:n, :n] / moving.
    Shares of an empty table, or of an empty moving part, are NaN."""
    a = check_table(table)
    n = a.shape[0] - 1
    total, core = float(a.sum()), a[:n, :n]
    moving = float(core.sum())
    k = np.arange(n)
    turn = np.bincount(((k[None, :] - k[:, None]) % n).reshape(-1), weights=core.reshape(-1), minlength=n)
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        hist = turn / moving if moving > 0 else np.full(n, nan)
        return {"total": total, "moving": moving, "turn_hist": hist, "forward": float(hist[0]),
                "reversal": float(hist[n // 2]) if n % 2 == 0 else nan,
                "persistence": float((hist * np.cos(2 * np.pi * k / n)).sum()),
                "stay_then_move": float(a[n, :n].sum()) / total if total > 0 else nan,
                "move_then_stay": float(a[:n, n].sum()) / total if total > 0 else nan,
                "stay_then_stay": float(a[n, n]) / total if total > 0 else nan,
                "transition": core / moving if moving > 0 else np.full((n, n), nan)}


def turn_comparison(table, human_table) -> dict:
    """The two comparison numbers of a transition table against the human one, in bits (jensen_shannon): "JSD_turn" between the
    turning-angle histograms and "JSD_transition" between the moving parts table[:n, :n], entry by entry"""
    a, h = check_table(table), check_table(human_table)
    if a.shape != h.shape:
        raise ValueError(f"tables of shapes {a.shape} and {h.shape}: one shape is required")
    n = a.shape[0] - 1
    return {"JSD_turn": jensen_shannon(turn_summary(a)["turn_hist"], turn_summary(h)["turn_hist"]),
            "JSD_transition": jensen_shannon(a[:n, :n], h[:n, :n])}
