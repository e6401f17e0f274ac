"""The argument checks and converters that more than one evaluation scorer uses: pure numpy, so every refusal comes before the device or
the library is touched.  A check that only one module uses, or that shares a name with another but differs in meaning (the two
_check_mix, scanpath_kde's _check_shape next to check_map_shape, the min_length of scanpath_likelihood._check_args), lives in its
module."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

_FIELDS = ("start_x", "start_y", "duration")
MAX_CELLS = 2048            # = sp_scan_likelihood_max_cells(), known here so that a refusal needs no library (held equal by the tests)
MAX_DIRECTIONS = 16         # = sp_scan_turn_max_directions(): two bin arrays [n + 1][256] in double next to three maps in 160 KB of LDS


def rows(sp) -> np.ndarray:
    """one scanpath -> float64 [n, ncol]: a structured fixation vector (start_x, start_y, duration) or an [n, >= 2] array"""
    a = np.asarray(sp)
    if a.dtype.names is not None:
        if any(f not in a.dtype.names for f in _FIELDS[:2]):
            raise ValueError(f"structured scanpath without start_x / start_y fields: {a.dtype.names}")
        cols = [f for f in _FIELDS if f in a.dtype.names]
        return np.stack([np.asarray(a[f], dtype=np.float64).reshape(-1) for f in cols], 1)
    a = a.astype(np.float64)
    if a.size == 0:
        return np.zeros((0, a.shape[-1] if a.ndim == 2 and a.shape[-1] >= 2 else 0))
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError(f"a scanpath is an [n, >= 2] array of (x, y[, duration]) rows, got shape {a.shape}")
    return a


def check_frame(frame_size) -> Tuple[float, float]:
    fh, fw = (float(v) for v in frame_size)
    if not (np.isfinite(fh) and np.isfinite(fw) and fh > 0 and fw > 0):
        raise ValueError(f"frame_size {tuple(frame_size)}: positive finite sizes are required")
    return fh, fw


def check_steps(max_steps) -> int:
    if max_steps is None or isinstance(max_steps, bool) or int(max_steps) != max_steps or int(max_steps) < 1:
        raise ValueError(f"max_steps {max_steps!r}: an integer >= 1")
    return int(max_steps)


def check_min_length(min_length) -> int:
    if min_length is None or isinstance(min_length, bool) or int(min_length) != min_length or int(min_length) < 0:
        raise ValueError(f"min_length {min_length!r}: an integer >= 0 (the sampler's)")
    return int(min_length)


def check_map(A: int, map_shape, *, max_cells: Optional[int] = None, max_side: Optional[int] = None) -> Tuple[int, int]:
    """(Hm, Wm) of a model output of A = 1 + Hm * Wm actions, within the calling kernel's limit on the cells or on a side"""
    if map_shape is None:
        if A != 1201:
            raise ValueError(f"map_shape is required for {A} actions (only 1201 = 1 + 30 * 40 has a default)")
        map_shape = (30, 40)
    Hm, Wm = (int(v) for v in map_shape)
    if Hm < 1 or Wm < 1 or Hm * Wm != A - 1:
        raise ValueError(f"map_shape {tuple(map_shape)} does not hold the {A - 1} cells of {A} actions")
    if max_cells is not None and Hm * Wm > max_cells:
        raise ValueError(f"map of {Hm * Wm} cells exceeds the kernel limit {max_cells}")
    if max_side is not None and (Hm > max_side or Wm > max_side):
        raise ValueError(f"map_shape {tuple(map_shape)}: a side exceeds the kernel limit {max_side}")
    return Hm, Wm


def check_map_shape(map_shape) -> Tuple[int, int]:
    """(Hm, Wm) of a map the caller names: two integers >= 1, at most MAX_CELLS cells"""
    try:
        Hm, Wm = (int(v) for v in map_shape)
        exact = all(int(v) == v for v in map_shape)
    except (TypeError, ValueError):
        raise ValueError(f"map_shape {map_shape!r}: (Hm, Wm), two integers >= 1, is required") from None
    if not exact or Hm < 1 or Wm < 1:
        raise ValueError(f"map_shape {tuple(map_shape)}: (Hm, Wm), two integers >= 1, is required")
    if Hm * Wm > MAX_CELLS:
        raise ValueError(f"map_shape {tuple(map_shape)}: a map of {Hm * Wm} cells exceeds the kernel limit {MAX_CELLS}")
    return Hm, Wm


def check_groups(groups, n, n_groups, what) -> Tuple[np.ndarray, int]:
    """(groups as int32 [n], n_groups): one group in [0, n_groups) per `what` (a scanpath, a row)"""
    from ._batch import check_index
    if n_groups is None or isinstance(n_groups, bool) or int(n_groups) != n_groups or int(n_groups) < 1:
        raise ValueError(f"n_groups {n_groups!r}: an integer >= 1")
    g = check_index(groups, int(n_groups), "group").reshape(-1)
    if len(g) != n:
        raise ValueError(f"one group per {what} is required: {len(g)} groups, {n} {what}s")
    return g.astype(np.int32), int(n_groups)


def check_directions(n_directions, limit: Optional[int] = None) -> int:
    """n_directions, an integer >= 1 and, for a kernel that bins by direction, at most its limit"""
    if n_directions is None or isinstance(n_directions, bool) or int(n_directions) != n_directions or int(n_directions) < 1:
        raise ValueError(f"n_directions {n_directions!r}: an integer >= 1")
    if limit is not None and int(n_directions) > limit:
        raise ValueError(f"n_directions {int(n_directions)}: exceeds the kernel limit {limit}")
    return int(n_directions)


def check_edges(amplitude_edges) -> np.ndarray:
    if amplitude_edges is None:
        raise ValueError("amplitude_edges is required: at least two increasing finite values, in pixels")
    e = np.asarray(amplitude_edges, dtype=np.float64).reshape(-1)
    if len(e) < 2 or not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError(f"amplitude_edges {e.tolist()}: at least two strictly increasing finite values are required")
    return e


def check_probs(probs) -> Tuple[int, int, int]:
    """(R, T, A) of the model's step distributions, a non-empty [R, T, A] tensor"""
    import torch
    if not isinstance(probs, torch.Tensor) or probs.dim() != 3 or min(probs.shape) < 1:
        raise ValueError("probs: a non-empty [R, T, A] tensor is required")
    R, T, A = (int(v) for v in probs.shape)
    return R, T, A
