"""The two reference points the likelihood scorers' bits are read against (scanpath_likelihood.py), on the device
(csrc/scankde.hip): the kernel-density centre-bias baseline of "IG" with a bandwidth chosen by leave-one-image-out
likelihood, and the human gold standard -- the other subjects' fixations on the same image as the predictor (Kümmerer, Wallis & Bethge
2015; Kümmerer, Bethge & Wallis 2022).  Both are Gaussian kernel sums between fixations with a leave-group-out rule.

    search = kde_bandwidth_search(scanpaths, image_groups, frame_size, map_shape, bandwidths=2.0 ** np.arange(2, 8, 0.5),
                                  uniform_mix=0.01, leave="image")                # {"LL": [K] mean bits, "best": the bandwidth, ...}
    base = kde_cell_baselines(scanpaths, image_groups, frame_size, map_shape, bandwidth=search["best"])   # [G, P]: baseline= of "IG"
    gold = kde_leave_out_likelihood(scanpaths, image_groups, frame_size, map_shape, bandwidth=16.0, uniform_mix=0.01,
                                    leave="scanpath_step", max_length=T)          # {"LL": [S, Tmax], "others", "n", "dropped"}

Frame (h, w), map (Hm, Wm), P = Hm * Wm cells; the cell of a fixation follows the pixel rule of scanpath_likelihood, and a fixation
outside the frame or with a non-finite coordinate is dropped: no source, NaN as a query, counted in "dropped".  Only the first
min(n, max_length) fixations of a scanpath count (max_length=None: all), t = the position in the recorded scanpath.  The cell kernel of a
source j at bandwidth b (pixels of the frame) is the softmax form of a Gaussian around it over the cell centres cx(col) = (col + 0.5)
w / Wm, cy(row) = (row + 0.5) h / Hm, separately on x and y:  wx_j(col) = exp(ax(col) - max ax) / sum_col exp(ax(col) - max ax),
ax(col) = -(cx(col) - x_j)^2 / (2 b^2), k_j(c) = wy_j(row) wx_j(col).  It sums to 1 over the map whatever b is (the mass that would
leave the frame is put back), is the one-hot of the nearest centre for b -> 0 and 1 / P for b -> inf.  The score of a query i at cell c:
q = sum_{j in A_i} k_j(c) / M, M = |A_i| (valid sources only), value log2(P ((1 - u) q + u / P)), u = uniform_mix; NaN for a dropped
query and for M = 0; no epsilon: with u = 0 a zero q scores -inf.  A_i by leave:
  "image"          the sources on all OTHER images of the call: the centre-bias score, = LL - IG of scanpath_likelihood under
                   kde_cell_baselines;
  "scanpath"       the sources of the OTHER scanpaths on the SAME image: the spatial gold standard;
  "scanpath_step"  as "scanpath", and at the same position t: the gold standard on the footing the model is scored on.
bandwidth / bandwidths and uniform_mix have no defaults.  One upload and one copy back per call; there is no CPU path, no map of more
than MAX_CELLS cells and no search over more than MAX_BANDWIDTHS bandwidths per call.  Not taken over: continuous pixel densities (the
density lives on the map's cells, as the model's does) and conditioning on the human scanpath history."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ... import hip
from ...hip import check
from . import _batch
from ._args import check_frame, rows
from ._batch import starts
from .scanpath_likelihood import MAX_CELLS

LEAVE = ("image", "scanpath", "scanpath_step")
MAX_BANDWIDTHS = 16         # = sp_scan_kde_max_bandwidths(), known here so that a refusal needs no library (held equal by the tests)


def _device() -> torch.device:
    return _batch.device("kernel density estimates run")


# ---- argument checks: every refusal comes before the device or the library is touched ---------------------------------------------------
def _check_bandwidths(bandwidths) -> np.ndarray:
    bw = np.asarray(bandwidths, dtype=np.float64).reshape(-1)
    if not 1 <= len(bw) <= MAX_BANDWIDTHS:
        raise ValueError(f"{len(bw)} bandwidths: between 1 and the kernel limit {MAX_BANDWIDTHS} per call")
    if not (np.isfinite(bw) & (bw > 0)).all():
        raise ValueError(f"bandwidth {bw[~(np.isfinite(bw) & (bw > 0))][0]!r}: finite numbers > 0 (pixels of the frame) are required")
    return np.ascontiguousarray(bw)


def _check_mix(uniform_mix) -> float:
    u = float(uniform_mix)
    if not (np.isfinite(u) and 0.0 <= u < 1.0):
        raise ValueError(f"uniform_mix {uniform_mix!r}: a finite number in [0, 1)")
    return u


def _check_shape(map_shape):
    Hm, Wm = (int(v) for v in map_shape)
    if Hm < 1 or Wm < 1:
        raise ValueError(f"map_shape {tuple(map_shape)}: positive sizes are required")
    if Hm * Wm > MAX_CELLS:
        raise ValueError(f"map of {Hm * Wm} cells exceeds the kernel limit {MAX_CELLS}")
    return Hm, Wm


class _Points:
    """the fixations that count, sorted by image (a stable sort of the scanpaths: within an image the caller's order), as the sections of
    the upload; pure numpy"""

    def __init__(self, scanpaths, image_groups, max_length, dense: bool):
        if max_length is not None and (isinstance(max_length, bool) or int(max_length) != max_length or int(max_length) < 1):
            raise ValueError(f"max_length {max_length!r}: None or an integer >= 1")
        arrs = [rows(sp)[:max_length] for sp in scanpaths]
        groups = _batch.check_index(list(image_groups), np.iinfo(np.int32).max, "image group").reshape(-1)
        if len(groups) != len(arrs):
            raise ValueError("one image group per scanpath is required")
        self.S = len(arrs)
        if dense:                                                                    # the ids need not be contiguous or sorted
            _, image = np.unique(groups, return_inverse=True)
            self.G = int(image.max()) + 1 if self.S else 0
        else:
            image, self.G = groups, int(groups.max()) + 1 if self.S else 0
        order = np.argsort(image, kind="stable")
        b = _batch.pack([arrs[s] for s in order], min_cols=2, limit=None)
        self.rows, self.ncol, self.N = b.rows, b.ncol, len(b.rows)
        self.n = np.zeros(self.S, dtype=np.int32)
        self.n[order] = b.counts
        self.Tmax = int(self.n.max()) if self.S else 0
        self.path = np.repeat(order, b.counts).astype(np.int32)
        self.step = (np.arange(self.N, dtype=np.int64) - np.repeat(b.starts, b.counts)).astype(np.int32)
        self.img = np.repeat(image[order], b.counts).astype(np.int32)
        per_image = np.bincount(self.img, minlength=self.G)
        self.img_start = np.concatenate([starts(per_image), [self.N]]).astype(np.int64)

    def blocks(self, K: int) -> np.ndarray:
        """[nblocks, 2] int32 (image, block of 256 (fixation, bandwidth) items of the image)"""
        nb = (np.diff(self.img_start) * K + 255) // 256
        image = np.repeat(np.arange(self.G), nb)
        return np.stack([image, np.arange(len(image)) - np.repeat(starts(nb), nb)], 1).astype(np.int32)

    def scatter(self, v, fill, dtype) -> np.ndarray:
        out = np.full((self.S, self.Tmax), fill, dtype=dtype)
        out[self.path, self.step] = v
        return out


def _launch(p: _Points, frame, shape, bw: np.ndarray, u: float, leave: int, scores: bool):
    """one upload, the launches of sp_scan_kde, -> (tables [G, K, P] on the device or None, Out of LL [N, K] / others / valid or None)"""
    (fh, fw), (Hm, Wm), K = frame, shape, len(bw)
    P = Hm * Wm
    dev = _device()
    L = hip.lib()
    if L.sp_scan_kde_max_bandwidths() != MAX_BANDWIDTHS or L.sp_scan_likelihood_max_cells() != MAX_CELLS:
        raise hip.HipError(f"kernel limits {L.sp_scan_kde_max_bandwidths()} / {L.sp_scan_likelihood_max_cells()}, this module expects "
                           f"{MAX_BANDWIDTHS} / {MAX_CELLS}")
    up = dict(rows=p.rows, path=p.path, step=p.step, img=p.img, img_start=p.img_start)
    if leave:
        up["blocks"] = p.blocks(K)
    buf, at = _batch.upload(up, dev)
    prep = torch.empty(max(p.N * K * 4, 1), dtype=torch.float64, device=dev)
    own = tables = nother = out = None
    if leave == 0:
        own = torch.empty(max(p.G * K * P, 1), dtype=torch.float64, device=dev)
        tables = torch.empty((p.G, K, P), dtype=torch.float64, device=dev)
        nother = torch.empty(max(p.G, 1), dtype=torch.int32, device=dev)
    if scores:
        out = _batch.Out(dict(LL=(np.float64, p.N * K), others=(np.int32, p.N), valid=(np.int32, p.N)), dev)
    ptr = lambda t: None if t is None else t.data_ptr()                                                    # noqa: E731
    optr = lambda name: out.ptr(name) if out is not None else None                                         # noqa: E731
    check(L.sp_scan_kde(at["rows"], at["path"], at["step"], at["img"], at["img_start"], at.get("blocks"), p.N, p.ncol, p.G,
                        len(up["blocks"]) if leave else 0, bw.ctypes.data, K, Hm, Wm, fw, fh, u, leave, ptr(prep), ptr(own),
                        ptr(nother), ptr(tables), optr("LL"), optr("others"), optr("valid"), hip.stream()),
          "sp_scan_kde")
    del buf
    return tables, out


def _leave_out(scanpaths, image_groups, frame_size, map_shape, bandwidths, uniform_mix, leave, max_length):
    """-> (_Points, LL [N, K], others [N], valid [N]) on the host, in the order of the points"""
    bw = _check_bandwidths(bandwidths)
    if uniform_mix is None:
        raise TypeError("the keyword uniform_mix is required (the share of the uniform density mixed into the estimate; it has no "
                        "default, and 0 is allowed: a zero density then scores -inf)")
    u = _check_mix(uniform_mix)
    if leave not in LEAVE:
        raise ValueError(f"leave {leave!r}: one of {LEAVE}")
    shape, frame = _check_shape(map_shape), check_frame(frame_size)
    p = _Points(scanpaths, image_groups, max_length, dense=True)
    if p.N == 0:                                                                     # nothing to score: no device
        return p, np.zeros((0, len(bw))), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    _, out = _launch(p, frame, shape, bw, u, LEAVE.index(leave), True)
    host = out.host()
    return p, host["LL"].reshape(p.N, len(bw)), host["others"], host["valid"]


# ---- public calls ---------------------------------------------------------------------------------------------------------------------------
def kde_cell_baselines(scanpaths, image_groups, frame_size, map_shape, *, bandwidth, max_length=None) -> torch.Tensor:
    """The kernel-density centre-bias baseline of "IG": row g = the sum of the cell kernels (module docstring) of the valid fixations of
    all scanpaths recorded on the OTHER images (image_groups[k] != g), unnormalised -- sp_scan_likelihood sum-normalises its baseline
    rows.  Arguments and layout as cell_baselines: [G, P] float64 on the device, G = max(image_groups) + 1, so it goes into baseline=
    of scanpath_likelihood / likelihood_evaluation / run_likelihood_loop.  The other images are summed directly (never total - own):
    with one image the row is exactly zero and IG scores NaN, and for bandwidth -> 0 the rows are cell_baselines' counts."""
    bw = _check_bandwidths([bandwidth] if np.ndim(bandwidth) == 0 else bandwidth)
    if len(bw) != 1:
        raise ValueError("kde_cell_baselines takes one bandwidth")
    shape, frame = _check_shape(map_shape), check_frame(frame_size)
    p = _Points(scanpaths, image_groups, max_length, dense=False)
    if p.G == 0:                                                                     # no scanpath, no image, no row
        return torch.zeros((0, shape[0] * shape[1]), dtype=torch.float64, device=_device())
    tables, _ = _launch(p, frame, shape, bw, 0.0, 0, False)
    return tables.reshape(p.G, shape[0] * shape[1])


def kde_leave_out_likelihood(scanpaths, image_groups, frame_size, map_shape, *, bandwidth, uniform_mix, leave, max_length=None
                             ) -> Dict[str, np.ndarray]:
    """The leave-out score (module docstring) of every fixation that counts.  scanpaths: S arrays [n, >= 2] of (x, y[, ..]) or
    structured fixation vectors, of any length; image_groups[s]: the image of scanpath s (any non-negative integers).  Returns {"LL":
    float64 [S, Tmax], NaN where nothing is scored; "others": int32 [S, Tmax] = M (0 for t >= n'); "n": int32 [S] = n' = min(n,
    max_length); "dropped": int32 [S]} in the caller's order, Tmax = the largest n'."""
    bw = _check_bandwidths([bandwidth] if np.ndim(bandwidth) == 0 else bandwidth)
    if len(bw) != 1:
        raise ValueError("kde_leave_out_likelihood takes one bandwidth (kde_bandwidth_search scores several)")
    p, LL, others, valid = _leave_out(scanpaths, image_groups, frame_size, map_shape, bw, uniform_mix, leave, max_length)
    return dict(LL=p.scatter(LL[:, 0], np.nan, np.float64), others=p.scatter(others, 0, np.int32), n=p.n,
                dropped=np.bincount(p.path[valid == 0], minlength=p.S).astype(np.int32))


def kde_bandwidth_search(scanpaths, image_groups, frame_size, map_shape, *, bandwidths, uniform_mix, leave, max_length=None) -> dict:
    """All K <= MAX_BANDWIDTHS bandwidths scored in one call (the pair pass reads its sources once).  Returns {"bandwidths": float64
    [K]; "LL": float64 [K], the mean leave-out score over the scored fixations; "sum": [K]; "count": how many fixations are scored (the
    same for every bandwidth); "best": the bandwidth of the largest mean, the first on a tie (NaN when nothing is scored)}."""
    bw = _check_bandwidths(bandwidths)
    p, LL, _, _ = _leave_out(scanpaths, image_groups, frame_size, map_shape, bw, uniform_mix, leave, max_length)
    sums, count = np.zeros(len(bw)), 0
    for k in range(len(bw)):
        v = p.scatter(LL[:, k], np.nan, np.float64)                                   # pooled in the caller's order
        v = v[~np.isnan(v)]
        sums[k], count = v.sum(), int(v.size)
    means = sums / count if count else np.full(len(bw), np.nan)
    return dict(bandwidths=bw, LL=means, sum=sums, count=count, best=float(bw[int(np.argmax(means))]) if count else float("nan"))
