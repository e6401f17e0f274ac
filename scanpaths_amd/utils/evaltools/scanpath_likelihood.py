"""Human scanpaths under the model's own step distributions, on the device (csrc/scanlik.hip): the scorers that read
what the model puts out -- a categorical distribution over 1 + Hm*Wm actions per decode step and a log-normal over the duration --
instead of scanpaths sampled from it (Kümmerer & Bethge 2021; Kümmerer, Bethge & Wallis 2022).

    res = scanpath_likelihood(probs, scanpaths, rows, frame_size, uniform_mix=0.01, metrics=("LL", "NSS", "AUC"))
    # {metric: float64 numpy [S, T] ("STOP": [S]), "n": int32 [S], "dropped": int32 [S]}
    base = cell_baselines(scanpaths, image_groups, frame_size, map_shape)          # [G, P] float64 on the device, for "IG"

Fixation t of a scanpath is compared with decode step t of row rows[s] of probs [R, T, 1 + P] (action 0 = terminate, action
1 + row * Wm + col = a cell, as models/sampling.py reads it); only the first min(n, T) fixations count, as the dataset's max_length
cut does.  The cell follows the pixel rule of fixation_maps; a fixation outside the frame or with a non-finite coordinate is dropped:
NaN in the spatial outputs, counted in "dropped".  With Z = the sum of the step's P cell probabilities, q' = (1 - u) p_c / Z + u / P:
  "LL"   log2(P q'): bits over the uniform density;
  "IG"   log2 q' - log2 b', b' the same mixture of row baseline_rows[s] of baseline [NB, P] (non-negative; sum-normalised by the
         kernel; a row with sum <= 0 scores NaN);
  "NSS"  (p_c - mean) / std over the step's P raw cell values, ddof 1 as NSS; NaN on a constant map or for P < 2;
  "AUC"  (#{p_c' < p_c} + 0.5 #{c' != c: p_c' == p_c}) / (P - 1) on the raw float32 values: exact;
  "DLL"  log2 of the log-normal density of the fixation's duration under log_normal_mu / log_normal_sigma2 [R, T] (the form of
         models/loss.py MLPLogNormalDistribution without its epsilon; NaN for d <= 0, non-finite d or sigma2 <= 0); it does not depend
         on the position, so a dropped fixation has one;
  "STOP" the log2-probability of the scanpath's length under the sampler's termination rule (terminate is masked for t < min_length):
         sum_{t = min_length}^{n' - 1} CONT[r, t] + (TERM[r, n'] if n' < T), n' = min(n, T), CONT = log2(Z / (Z + p_0)), TERM =
         log2(p_0 / (Z + p_0)); -inf for n' < min_length and n' < T.
Per-fixation outputs are NaN for t >= min(n, T); "n" = min(n, T).  No epsilon goes inside any logarithm: uniform_mix is the only
regulariser, it has no default, and with 0 a zero probability scores -inf, reported as such.  One upload, one launch and one copy back
per call; probs, mu and sigma2 stay on the device.  There is no CPU path, no map of more than MAX_CELLS cells and no conditioning on
earlier human fixations (the model has none).  The two reference points the bits are read against -- the kernel-density centre-bias
baseline for "IG" (kde_cell_baselines, in place of cell_baselines' raw histogram) and the human gold-standard row -- are
scanpath_kde.py's."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr
from . import _batch
from ._args import MAX_CELLS, check_frame, check_map, rows as _rows  # (rows is an argument of scanpath_likelihood)
from ._batch import MAX_FIXATIONS, check_index, pack, starts  # noqa: F401  (MAX_FIXATIONS re-exported)

METRICS = ("LL", "IG", "NSS", "AUC", "DLL", "STOP")
_PER_FIXATION = METRICS[:5]


def _device() -> torch.device:
    return _batch.device("scanpath likelihoods run")


# ---- argument checks: every refusal comes before the device or the library is touched ---------------------------------------------------
def _check_args(metrics, uniform_mix, min_length) -> Tuple[Tuple[str, ...], float, int]:
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    unknown = [m for m in metrics if m not in METRICS]
    if unknown:
        raise ValueError(f"unknown likelihood metric {unknown[0]!r}: one of {METRICS}")
    if len(set(metrics)) != len(metrics):
        raise ValueError(f"repeated likelihood metric in {metrics}")
    if not metrics:
        raise ValueError("no likelihood metric asked for")
    if uniform_mix is None:
        if "LL" in metrics or "IG" in metrics:
            raise TypeError("LL and IG need the keyword uniform_mix (the share of the uniform density mixed into both distributions; it "
                            "has no default, and 0 is allowed: a zero probability then scores -inf)")
        u = 0.0
    else:
        u = float(uniform_mix)
        if not (np.isfinite(u) and 0.0 <= u < 1.0):
            raise ValueError(f"uniform_mix {uniform_mix!r}: a finite number in [0, 1)")
    if isinstance(min_length, bool) or int(min_length) != min_length or int(min_length) < 0:
        raise ValueError(f"min_length {min_length!r}: an integer >= 0")
    return metrics, u, int(min_length)


def _stop(cont: np.ndarray, term: np.ndarray, row: np.ndarray, n: np.ndarray, min_length: int) -> np.ndarray:
    """STOP of every scanpath from CONT / TERM [R, T]; the sums run left to right in index order (np.cumsum accumulates that way)"""
    R, T = cont.shape
    run = np.zeros((R, 1))                                   # run[r, k] = CONT[r, min_length] + .. + CONT[r, min_length + k - 1]
    if min_length < T:
        run = np.concatenate([run, np.cumsum(cont[:, min_length:], axis=1)], 1)
    stop = run[row, np.maximum(n - min_length, 0)]
    ends = n < T
    stop[ends] = stop[ends] + term[row[ends], n[ends]]
    stop[ends & (n < min_length)] = -np.inf
    return stop


# ---- public calls ---------------------------------------------------------------------------------------------------------------------------
def scanpath_likelihood(probs, scanpaths, rows, frame_size, *, uniform_mix=None, metrics=("LL", "NSS", "AUC"), map_shape=None,
                        baseline=None, baseline_rows=None, log_normal_mu=None, log_normal_sigma2=None, min_length=0
                        ) -> Dict[str, np.ndarray]:
    """probs: device tensor [R, T, 1 + P] (any float dtype; detached and read as float32); scanpaths: S arrays [n <= 64, >= 2] of
    (x, y[, duration]) or structured fixation vectors, in the frame frame_size = (height, width); rows[s]: the row of probs that scores
    scanpath s, in any order.  metrics: any of METRICS (module docstring); uniform_mix is required for "LL" / "IG"; map_shape =
    (Hm, Wm) defaults to (30, 40) for 1201 actions only; "IG" needs baseline [NB, P] (device tensor or array) and baseline_rows [S];
    "DLL" needs log_normal_mu / log_normal_sigma2 [R, T] and a duration column; min_length: the sampler's, for "STOP".  Returns
    {metric: float64 numpy [S, T] ("STOP": [S]), "n": int32 [S] = min(n, T), "dropped": int32 [S]} in the caller's order."""
    metrics, u, min_length = _check_args(metrics, uniform_mix, min_length)
    if not isinstance(probs, torch.Tensor) or probs.dim() != 3 or min(probs.shape) < 1:
        raise ValueError("probs: a non-empty [R, T, A] tensor is required")
    R, T, A = (int(v) for v in probs.shape)
    Hm, Wm = check_map(A, map_shape, max_cells=MAX_CELLS)
    P = Hm * Wm
    fh, fw = check_frame(frame_size)
    want_ig, want_dll, want_stop = "IG" in metrics, "DLL" in metrics, "STOP" in metrics
    if want_ig and (baseline is None or baseline_rows is None):
        raise TypeError("IG needs the keywords baseline ([NB, P]) and baseline_rows (one row index per scanpath)")
    if want_dll and (log_normal_mu is None or log_normal_sigma2 is None):
        raise TypeError("DLL needs the keywords log_normal_mu and log_normal_sigma2 ([R, T])")
    b = pack([_rows(sp) for sp in scanpaths], min_cols=3 if want_dll else 2)
    S = len(b.counts)
    row = check_index(rows, R, "row").reshape(-1)
    if len(row) != S:
        raise ValueError("one row per scanpath is required")
    up = {}
    if want_ig:
        if not isinstance(baseline, torch.Tensor):
            baseline = np.asarray(baseline, dtype=np.float64)
        if len(baseline.shape) != 2 or baseline.shape[0] < 1 or baseline.shape[1] != P:
            raise ValueError(f"baseline of shape {tuple(baseline.shape)}: [NB, {P}] is required")
        brow = check_index(baseline_rows, int(baseline.shape[0]), "baseline row").reshape(-1)
        if len(brow) != S:
            raise ValueError("one baseline row per scanpath is required")
        up["baseline_rows"] = brow.astype(np.int32)
        if not (isinstance(baseline, torch.Tensor) and baseline.is_cuda):            # a host baseline travels with the one upload
            up["baseline"] = np.ascontiguousarray(baseline.numpy() if isinstance(baseline, torch.Tensor) else baseline, dtype=np.float64)
    if want_dll and not (tuple(log_normal_mu.shape) == tuple(log_normal_sigma2.shape) == (R, T)):
        raise ValueError(f"log_normal_mu / log_normal_sigma2 of shapes {tuple(log_normal_mu.shape)} / {tuple(log_normal_sigma2.shape)}: "
                         f"[{R}, {T}] is required")
    n = np.minimum(b.counts, T).astype(np.int32)
    if S == 0:
        res = {m: np.zeros(0 if m == "STOP" else (0, T), dtype=np.float64) for m in metrics}
        return dict(res, n=n, dropped=np.zeros(0, dtype=np.int32))

    dev = _device()
    L = hip.lib()
    _batch.check_limits(L)
    if L.sp_scan_likelihood_max_cells() != MAX_CELLS:
        raise hip.HipError(f"sp_scan_likelihood_max_cells() = {L.sp_scan_likelihood_max_cells()}, this module expects {MAX_CELLS}")
    row_n = np.bincount(row, minlength=R).astype(np.int32)                             # the scanpaths of a row, next to each other
    up = b.sections(row_first=starts(row_n).astype(np.int32), row_n=row_n, order=np.argsort(row, kind="stable").astype(np.int32), **up)
    buf, at = _batch.upload(up, dev)
    p = probs.detach().to(torch.float32).contiguous()
    mu = log_normal_mu.detach().to(torch.float32).contiguous() if want_dll else None
    s2 = log_normal_sigma2.detach().to(torch.float32).contiguous() if want_dll else None
    base = baseline.detach().to(torch.float64).contiguous() if want_ig and "baseline" not in at else None
    sections = {m: (np.float64, S * T) for m in _PER_FIXATION if m in metrics}
    if want_stop:
        sections.update(CONT=(np.float64, R * T), TERM=(np.float64, R * T))
    sections["dropped"] = (np.int32, S)
    out = _batch.Out(sections, dev)
    check(L.sp_scan_likelihood(ptr(p), ptr(mu), ptr(s2), at.get("baseline", ptr(base)), at.get("baseline_rows"), at["rows"], at["starts"], at["counts"],
                               at["row_first"], at["row_n"], at["order"], R, T, Hm, Wm, S, b.ncol, fw, fh, u, out.ptr("LL"), out.ptr("IG"),
                               out.ptr("NSS"), out.ptr("AUC"), out.ptr("DLL"), out.ptr("CONT"), out.ptr("TERM"), out.ptr("dropped"),
                               hip.stream()), "sp_scan_likelihood")
    host = out.host()
    res = {}
    for m in metrics:
        res[m] = (_stop(host["CONT"].reshape(R, T), host["TERM"].reshape(R, T), row, n.astype(np.int64), min_length) if m == "STOP"
                  else host[m].reshape(S, T))
    return dict(res, n=n, dropped=host["dropped"])


def cell_baselines(scanpaths, image_groups, frame_size, map_shape) -> torch.Tensor:
    """The centre-prior baseline of "IG" at map resolution: row g = the cell counts of the fixations of all scanpaths recorded on the
    OTHER images (image_groups[k] != g) -- what can be said about where people look without seeing image g.  scanpaths /
    image_groups / frame_size as fixation_maps takes them, scanpaths of any length.  Returns [G, P] float64 on the device (P =
    Hm * Wm, G = max(image_groups) + 1); the counts are integers, hence exact.  With one image the row is zero and IG scores NaN."""
    from .saliency_maps import fixation_maps
    maps, _ = fixation_maps(scanpaths, image_groups, frame_size, output_shape=map_shape, weight="count")
    flat = maps.reshape(maps.shape[0], -1)
    return flat.sum(0, keepdim=True) - flat
