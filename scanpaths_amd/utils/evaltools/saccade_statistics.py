"""Saccade statistics on the device (csrc/scansaccade.hip): how scanpaths move -- the distribution of saccade amplitudes,
of saccade directions, their joint distribution and the share of "saccades" that stay in the same cell (Le Meur & Liu 2015; Tatler &
Vincent 2009) -- for scanpaths that exist and, in closed form, for the model's own step distributions:

    res = saccade_counts(scanpaths, groups, n_groups, frame_size, map_shape, max_steps=16)       # humans, samples
    # {"counts": int64 [G, 2 Hm - 1, 2 Wm - 1], "saccades": int32 [S], "dropped": int32 [S]}
    res = saccade_expectation(probs, row_groups, n_groups, min_length=1, max_steps=16)           # the model itself, without sampling
    # {"E": float64 [G, 2 Hm - 1, 2 Wm - 1], "saccades": float64 [R], "bad": int32 [R]}
    s = saccade_summary(res["E"][0], frame_size, amplitude_edges=edges, n_directions=8)

Both sides of every comparison live on ONE displacement lattice.  A fixation is read as the action-map cell it falls in (the pixel rule
of fixation_maps / scanpath_likelihood: col = floor(x Wm / frame_w), row = floor(y Hm / frame_h)); a saccade is the cell displacement
(dr, dc) = (row(f_{t+1}) - row(f_t), col(f_{t+1}) - col(f_t)), held at entry [dr + Hm - 1, dc + Wm - 1] of a (2 Hm - 1) x (2 Wm - 1)
array; frame_size = (height, width).  All derived statistics come from such a lattice by the routines below, so humans, samples and the
model are binned by the same code.
saccade_counts: only the first min(n, max_steps) fixations of a scanpath count; a fixation outside the frame or with a non-finite
coordinate is dropped ("dropped"), and a saccade counts iff both of its fixations are kept -- nothing bridges a dropped fixation.
"saccades" = the number counted per scanpath.  Integers, hence exact and independent of any order.
saccade_expectation: probs [R, T, 1 + P] are the model's eval-mode step distributions (action 0 = terminate, action 1 + row * Wm + col
= a cell).  The decoder is not conditioned on sampled fixations, so two consecutive fixations of one sample are independent given the
image, and under the sampler's rule (terminate masked for t < min_length, the first terminate ends the scanpath) the expected number of
saccades with displacement d is E[d] = sum_t A_t sum_i c_t(i) c_{t+1}(i + d): a cross-correlation of consecutive step maps times the
probability A_t of still running -- no sampling noise.  Per step t < Tm = min(T, max_steps), in float64: Z = the sum of the P cells; D =
Z + p_0 for t >= min_length, else Z; q = p_0 / D for t >= min_length, else 0; c(i) = p_{1+i} / D; A_0 = 1, A_{t+1} = A_t (1 - q_t).
"saccades"[r] = sum_t A_t (1 - q_t)(1 - q_{t+1}), the lattice total of row r.  A row with a D that is zero or not finite at some t < Tm
is bad: "bad" 1, "saccades" NaN, and it adds nothing to its group.  max_steps and min_length have no defaults: they are the
evaluation's and the sampler's, and a silent mismatch changes every number.  Maps of at most 2048 cells (two maps in double fit in 32 KB
of LDS).  One upload, two launches and one copy back per call; probs stays on the device; R (2 Hm - 1)(2 Wm - 1) doubles of device
scratch per call.  There is no CPU path.
lattice_vectors, saccade_summary, jensen_shannon, wasserstein_amplitude and saccade_comparison are pure numpy and take integer counts or
expectations alike."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _batch
from ._args import MAX_CELLS, check_directions, check_edges, check_frame, check_map, check_map_shape, check_min_length, check_probs, check_steps
from ._batch import MAX_FIXATIONS  # noqa: F401  (re-exported)
from ._grouped import grouped_counts, grouped_expectation


def _device() -> torch.device:
    return _batch.device("saccade statistics run")


# ---- argument checks: every refusal comes before the device or the library is touched ---------------------------------------------------
def _check_lattice(lattice) -> Tuple[np.ndarray, int, int]:
    a = np.asarray(lattice)
    if a.ndim != 2 or a.shape[0] % 2 != 1 or a.shape[1] % 2 != 1:
        raise ValueError(f"a displacement lattice is a [2 Hm - 1, 2 Wm - 1] array, got shape {a.shape}")
    return a.astype(np.float64), (a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2


# ---- device calls -------------------------------------------------------------------------------------------------------------------------
def saccade_counts(scanpaths, groups, n_groups, frame_size, map_shape, *, max_steps) -> Dict[str, np.ndarray]:
    """scanpaths: S arrays [n <= 64, >= 2] of (x, y, ...) or structured fixation vectors; groups [S] in [0, n_groups): the lattice each
    scanpath is counted into (an empty group stays zero); frame_size = (height, width); map_shape = (Hm, Wm), at most 2048 cells.
    Returns {"counts": int64 [n_groups, 2 Hm - 1, 2 Wm - 1], "saccades": int32 [S], "dropped": int32 [S]} (module docstring)."""
    max_steps = check_steps(max_steps)
    Hm, Wm = check_map_shape(map_shape)
    return grouped_counts("sp_scan_saccade_counts", _device, scanpaths, groups, n_groups, check_frame(frame_size), (Hm, Wm), max_steps,
                          shape=(2 * Hm - 1, 2 * Wm - 1), unit="saccades")


def saccade_expectation(probs, row_groups, n_groups, *, min_length, max_steps, map_shape=None) -> Dict[str, np.ndarray]:
    """probs: device tensor [R, T, 1 + P] (any float dtype; detached and read as float32); row_groups [R] in [0, n_groups): the lattice
    each row is added into, in ascending row index; min_length: the sampler's (required); max_steps: only the first max_steps steps
    count (required); map_shape = (Hm, Wm) defaults to (30, 40) for 1201 actions only.
    Returns {"E": float64 [n_groups, 2 Hm - 1, 2 Wm - 1], "saccades": float64 [R], "bad": int32 [R]} (module docstring)."""
    min_length, max_steps = check_min_length(min_length), check_steps(max_steps)
    R, _, A = check_probs(probs)
    Hm, Wm = check_map(A, map_shape, max_cells=MAX_CELLS)
    shape = (2 * Hm - 1, 2 * Wm - 1)
    return grouped_expectation("sp_scan_saccade_expectation", _device, probs, (Hm, Wm), row_groups, n_groups, min_length, max_steps,
                               shape=shape, work=R * shape[0] * shape[1], name="E", unit="saccades")


# ---- pure numpy, on one lattice -----------------------------------------------------------------------------------------------------------
def lattice_vectors(map_shape, frame_size) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(dx, dy, amplitude), each float64 [2 Hm - 1, 2 Wm - 1]: the pixel displacement of every lattice entry, dx = dc * frame_w / Wm and
    dy = dr * frame_h / Hm (y pointing down, as stored), and its length sqrt(dx * dx + dy * dy)"""
    Hm, Wm = check_map_shape(map_shape)
    fh, fw = check_frame(frame_size)
    dy = np.arange(-(Hm - 1), Hm, dtype=np.float64) * fh / Hm
    dx = np.arange(-(Wm - 1), Wm, dtype=np.float64) * fw / Wm
    dx, dy = np.broadcast_to(dx[None, :], (2 * Hm - 1, 2 * Wm - 1)).copy(), np.broadcast_to(dy[:, None], (2 * Hm - 1, 2 * Wm - 1)).copy()
    return dx, dy, np.sqrt(dx * dx + dy * dy)


def direction_sectors(map_shape, frame_size, n_directions) -> np.ndarray:
    """int64 [2 Hm - 1, 2 Wm - 1]: the direction sector of every lattice entry, -1 for the zero displacement.  Sector k of n is centred on
    the angle 2 pi k / n of atan2(dy, dx): k = int(floor(atan2(dy, dx) * n / (2 pi) + 0.5)) mod n, evaluated in that order in float64 --
    so a vector exactly on the boundary between sectors k and k + 1 (the expression is k + 1 exactly) belongs to sector k + 1, the one
    at the larger angle (with y pointing down: clockwise on the screen)."""
    n = check_directions(n_directions)
    dx, dy, _ = lattice_vectors(map_shape, frame_size)
    k = np.floor(np.arctan2(dy, dx) * n / (2 * np.pi) + 0.5).astype(np.int64) % n
    k[(dx == 0) & (dy == 0)] = -1
    return k


def saccade_summary(lattice, frame_size, *, amplitude_edges, n_directions) -> dict:
    """The descriptive statistics of one displacement lattice (integer counts or expectations; the map shape is read off its shape).
    amplitude_edges: >= 2 strictly increasing pixel values; n_directions >= 1; both required.  Returns
      "total": the lattice's mass (the number of saccades);  "stay": the share of zero displacements;  "mean_amplitude": the mean
      pixel length, zero displacements included;  "amplitude_hist" float64 [len(edges) - 1]: the share with edges[k] <= amplitude <
      edges[k + 1] (half-open; an amplitude below edges[0] is in no bin);  "amplitude_overflow": the share at or above the last edge;
      "direction_hist" float64 [n_directions]: the share, among the NON-ZERO displacements, of every sector of direction_sectors -- a
      vector exactly on a sector boundary goes to floor(atan2(dy, dx) * n / (2 pi) + 0.5) mod n, the sector at the larger angle.
    Shares of an empty lattice (and direction shares of a stay-only one) are NaN."""
    edges, n = check_edges(amplitude_edges), check_directions(n_directions)
    a, Hm, Wm = _check_lattice(lattice)
    fh, fw = check_frame(frame_size)
    _, _, amp = lattice_vectors((Hm, Wm), (fh, fw))
    total = float(a.sum())
    flat, ampf = a.reshape(-1), amp.reshape(-1)
    which = np.searchsorted(edges, ampf, side="right") - 1                 # edges[k] <= amplitude < edges[k + 1]; -1 below, len - 1 at or above
    inside = (which >= 0) & (which < len(edges) - 1)
    hist = np.bincount(which[inside], weights=flat[inside], minlength=len(edges) - 1)
    over = float(flat[which == len(edges) - 1].sum())
    sector = direction_sectors((Hm, Wm), (fh, fw), n).reshape(-1)
    moving = sector >= 0
    dirs = np.bincount(sector[moving], weights=flat[moving], minlength=n)
    moved = float(flat[moving].sum())
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"total": total, "stay": float(a[Hm - 1, Wm - 1]) / total if total > 0 else nan,
                "mean_amplitude": float((flat * ampf).sum()) / total if total > 0 else nan,
                "amplitude_hist": hist / total if total > 0 else np.full(len(edges) - 1, nan),
                "amplitude_overflow": over / total if total > 0 else nan,
                "direction_hist": dirs / moved if moved > 0 else np.full(n, nan)}


def jensen_shannon(p, q) -> float:
    """The Jensen-Shannon divergence in bits between two non-negative arrays of one shape, each normalised to sum 1 first; 0 log 0 = 0.
    0 for identical inputs, 1 for disjoint ones; NaN when either side has no mass (or a non-finite one)."""
    p, q = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(q, dtype=np.float64).reshape(-1)
    if p.shape != q.shape:
        raise ValueError(f"inputs of {p.size} and {q.size} entries: equal shapes are required")
    sp, sq = float(p.sum()), float(q.sum())
    if not (np.isfinite(sp) and np.isfinite(sq) and sp > 0 and sq > 0):
        return float("nan")
    p, q = p / sp, q / sq
    m = (p + q) / 2.0

    def half(a):
        nz = a > 0
        return float((a[nz] * np.log2(a[nz] / m[nz])).sum())

    return 0.5 * half(p) + 0.5 * half(q)


def wasserstein_amplitude(lattice_a, lattice_b, frame_size) -> float:
    """The exact 1-D Wasserstein-1 distance, in pixels, between the amplitude distributions of two lattices of one shape, on the
    lattice's own amplitude values: the sum over the sorted distinct amplitudes v_j of |CDF_a(v_j) - CDF_b(v_j)| * (v_{j+1} - v_j).
    NaN when either lattice has no mass."""
    a, Hm, Wm = _check_lattice(lattice_a)
    b, Hb, Wb = _check_lattice(lattice_b)
    if (Hm, Wm) != (Hb, Wb):
        raise ValueError(f"lattices of shapes {a.shape} and {b.shape}: one shape is required")
    _, _, amp = lattice_vectors((Hm, Wm), frame_size)
    sa, sb = float(a.sum()), float(b.sum())
    if not (np.isfinite(sa) and np.isfinite(sb) and sa > 0 and sb > 0):
        return float("nan")
    values, where = np.unique(amp.reshape(-1), return_inverse=True)
    where = where.reshape(-1)
    pa = np.bincount(where, weights=a.reshape(-1), minlength=len(values)) / sa
    pb = np.bincount(where, weights=b.reshape(-1), minlength=len(values)) / sb
    gap = np.abs(np.cumsum(pa) - np.cumsum(pb))[:-1]
    return float((gap * np.diff(values)).sum())


def saccade_comparison(lattice, human_lattice, frame_size, *, amplitude_edges, n_directions) -> dict:
    """The four comparison numbers of a lattice against the human one: "JSD_lattice" (the joint distribution, entry by entry),
    "JSD_amplitude" (the amplitude histogram with its overflow as a last bin), "JSD_direction" (the direction histogram), all in bits,
    and "W1_amplitude" in pixels"""
    kw = dict(amplitude_edges=amplitude_edges, n_directions=n_directions)
    s, h = saccade_summary(lattice, frame_size, **kw), saccade_summary(human_lattice, frame_size, **kw)
    return {"JSD_lattice": jensen_shannon(lattice, human_lattice),
            "JSD_amplitude": jensen_shannon(np.r_[s["amplitude_hist"], s["amplitude_overflow"]], np.r_[h["amplitude_hist"], h["amplitude_overflow"]]),
            "JSD_direction": jensen_shannon(s["direction_hist"], h["direction_hist"]),
            "W1_amplitude": wasserstein_amplitude(lattice, human_lattice, frame_size)}
