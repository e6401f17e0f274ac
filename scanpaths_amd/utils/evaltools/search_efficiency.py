"""Target-search efficiency on the device (csrc/scansearch.hip): did a scanpath reach the target, and how fast -- the
target-fixation probability (TFP) as a function of the number of fixations made, its area, the probability mismatch against the human
curve and the scanpath ratio (Yang et al. 2020; Mondal et al. 2023) -- in two forms:

    res = target_hits(scanpaths, boxes, max_steps=6)                          # scanpaths that exist: humans, samples
    # {"hit": int32 [S], "path": float64 [S], "SPR": float64 [S], "n": int32 [S]}
    curve = search_curve(res["hit"], 6); auc = tfp_auc(curve); pm = probability_mismatch(curve, human_curve)
    res = target_hit_probability(probs, boxes, box_rows, frame_size, min_length=1)    # the model itself, without sampling
    # {"MASS", "HIT", "TFP": float64 [NB, T], "cells": int32 [NB]}

A box is (x_min, y_min, x_max, y_max) in pixels of the frame, HALF-OPEN: a point is inside iff x_min <= x < x_max and y_min <= y <
y_max.  There is no segmentation-mask form of the target.
target_hits: only the first min(n, max_steps) fixations of a scanpath count ("n"); "hit" = the index of the first fixation inside its
box, -1 for none; "path" = the length of the scanpath up to the hit, the distances of consecutive fixations added left to right (0 for
a hit at 0, NaN without a hit); "SPR" = the scanpath ratio |fixation 0 - box centre| / path, NOT clipped at 1 (1.0 for a hit at 0, NaN
without a hit).  A fixation with a non-finite coordinate is never inside, and before the hit it makes "path" and "SPR" NaN.
target_hit_probability: probs [R, T, 1 + P] are the model's eval-mode step distributions (action 0 = terminate, action 1 + row * Wm +
col = a cell); the decoder is not conditioned on sampled fixations, so they are all there is to know about its samples.  Under the
sampler's rule (models/sampling.py: terminate is masked for t < min_length, the first terminate ends the scanpath, a cell becomes the
pixel of its centre) the probability that the FIRST fixation inside a box is fixation t has a closed form.  Cell (r, c) belongs to a
box iff the pixel the sampler emits for it -- in the sampler's float32 arithmetic -- is inside; "cells" counts them.  Per step, in
float64: Z = the sum of the P cells; D = Z + p_0 for t >= min_length, else Z; q = p_0 / D for t >= min_length, else 0; "MASS" m = (the
sum of the box's cells) / D; A_0 = 1, A_{t+1} = A_t ((1 - q) - m); "HIT"_t = A_t m_t; "TFP"_t = HIT_0 + .. + HIT_t.  D = 0 or a NaN gives
NaN at that step and every later step of the box.  Box b is read against row box_rows[b]; a row may have any number of boxes.
min_length has no default: it is the sampler's, and a silent mismatch changes every number.  Maps of any size up to 1024 x 1024.
One upload, one launch and one copy back per call; probs stays on the device.  There is no CPU path.  search_curve, tfp_auc and
probability_mismatch are pure numpy: TFP-AUC is the plain sum of the cumulative curve and the mismatch the plain sum of absolute
differences, as the papers describe them."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr
from . import _batch
from ._args import check_frame, check_map, check_min_length, check_steps, rows
from ._batch import MAX_FIXATIONS, check_index, pack  # noqa: F401  (MAX_FIXATIONS re-exported)

MAX_SIDE = 1024             # Hm, Wm at most this (the launcher's refusal, known here so that it needs no library)


def _device() -> torch.device:
    return _batch.device("search efficiency runs")


# ---- argument checks: every refusal comes before the device or the library is touched ---------------------------------------------------
def _check_boxes(boxes, n=None) -> np.ndarray:
    box = np.asarray(boxes, dtype=np.float64)
    if box.size == 0:
        box = box.reshape(0, 4)
    if box.ndim != 2 or box.shape[1] != 4:
        raise ValueError(f"boxes of shape {box.shape}: [N, 4] rows of (x_min, y_min, x_max, y_max) are required")
    if n is not None and len(box) != n:
        raise ValueError(f"one box per scanpath is required: {len(box)} boxes, {n} scanpaths")
    if not np.isfinite(box).all():
        raise ValueError("non-finite box value")
    return np.ascontiguousarray(box)


# ---- device calls -------------------------------------------------------------------------------------------------------------------------
def target_hits(scanpaths, boxes, *, max_steps) -> Dict[str, np.ndarray]:
    """scanpaths: S arrays [n <= 64, >= 2] of (x, y, ...) or structured fixation vectors; boxes [S, 4], one per scanpath, finite.
    Returns {"hit": int32 [S], "path", "SPR": float64 [S], "n": int32 [S] = min(n, max_steps)} (module docstring)."""
    max_steps = check_steps(max_steps)
    b = pack([rows(sp)[:, :2] for sp in scanpaths], min_cols=2)
    S = len(b.counts)
    box = _check_boxes(boxes, S)
    n = np.minimum(b.counts, max_steps).astype(np.int32)
    if S == 0:
        return {"hit": np.zeros(0, np.int32), "path": np.zeros(0), "SPR": np.zeros(0), "n": n}
    dev = _device()
    L = hip.lib()
    _batch.check_limits(L)
    buf, at = _batch.upload(b.sections(box=box), dev)
    out = _batch.Out({"path": (np.float64, S), "SPR": (np.float64, S), "hit": (np.int32, S)}, dev)
    check(L.sp_scan_target_hits(at["rows"], b.ncol, at["starts"], at["counts"], at["box"], S, max_steps, out.ptr("hit"), out.ptr("path"),
                                out.ptr("SPR"), hip.stream()), "sp_scan_target_hits")
    host = out.host()
    return {"hit": host["hit"], "path": host["path"], "SPR": host["SPR"], "n": n}


def target_hit_probability(probs, boxes, box_rows, frame_size, *, min_length, map_shape=None) -> Dict[str, np.ndarray]:
    """probs: device tensor [R, T, 1 + P] (any float dtype; detached and read as float32); boxes [NB, 4] in the frame frame_size =
    (height, width), finite; box_rows[b]: the row of probs box b is read against; min_length: the sampler's (required); map_shape =
    (Hm, Wm) defaults to (30, 40) for 1201 actions only.  Returns {"MASS", "HIT", "TFP": float64 [NB, T], "cells": int32 [NB]}."""
    min_length = check_min_length(min_length)
    if not isinstance(probs, torch.Tensor) or probs.dim() != 3 or min(probs.shape) < 1:
        raise ValueError("probs: a non-empty [R, T, A] tensor is required")
    R, T, A = (int(v) for v in probs.shape)
    Hm, Wm = check_map(A, map_shape, max_side=MAX_SIDE)
    fh, fw = check_frame(frame_size)
    box = _check_boxes(boxes)
    NB = len(box)
    row = check_index(box_rows, R, "box row").reshape(-1)
    if len(row) != NB:
        raise ValueError(f"one row per box is required: {len(row)} rows, {NB} boxes")
    if NB == 0:
        return dict({m: np.zeros((0, T)) for m in ("MASS", "HIT", "TFP")}, cells=np.zeros(0, np.int32))
    dev = _device()
    L = hip.lib()
    buf, at = _batch.upload({"box": box, "box_row": row.astype(np.int32)}, dev)
    p = probs.detach().to(torch.float32).contiguous()
    out = _batch.Out({"MASS": (np.float64, NB * T), "HIT": (np.float64, NB * T), "TFP": (np.float64, NB * T), "cells": (np.int32, NB)}, dev)
    check(L.sp_scan_target_mass(ptr(p), at["box"], at["box_row"], R, T, Hm, Wm, NB, fw, fh, min_length, out.ptr("MASS"), out.ptr("HIT"),
                                out.ptr("TFP"), out.ptr("cells"), hip.stream()), "sp_scan_target_mass")
    host = out.host()
    return {"MASS": host["MASS"].reshape(NB, T), "HIT": host["HIT"].reshape(NB, T), "TFP": host["TFP"].reshape(NB, T),
            "cells": host["cells"]}


# ---- pure numpy ---------------------------------------------------------------------------------------------------------------------------
def search_curve(hit, max_steps) -> np.ndarray:
    """float64 [max_steps]: the share of scanpaths with 0 <= hit <= k, for k = 0 .. max_steps - 1 (NaN without scanpaths)"""
    max_steps = check_steps(max_steps)
    hit = np.asarray(hit, dtype=np.int64).reshape(-1)
    if not len(hit):
        return np.full(max_steps, np.nan)
    return hit_counts(hit, max_steps) / float(len(hit))


def hit_counts(hit, max_steps) -> np.ndarray:
    """float64 [max_steps]: the number of scanpaths with 0 <= hit <= k -- the numerators of search_curve (integers, hence exact)"""
    hit = np.asarray(hit, dtype=np.int64).reshape(-1)
    first = np.bincount(hit[(hit >= 0) & (hit < max_steps)], minlength=max_steps)
    return np.cumsum(first).astype(np.float64)


def tfp_auc(curve) -> float:
    """the area under a cumulative hit curve: the plain sum of its values"""
    return float(np.sum(np.asarray(curve, dtype=np.float64)))


def probability_mismatch(curve, human_curve) -> float:
    """the sum of absolute differences between a model's curve and the human one (equal lengths)"""
    a, b = np.asarray(curve, dtype=np.float64).reshape(-1), np.asarray(human_curve, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError(f"curves of {len(a)} and {len(b)} steps: equal lengths are required")
    return float(np.sum(np.abs(a - b)))
