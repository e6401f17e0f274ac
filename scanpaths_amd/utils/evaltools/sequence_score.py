"""Sequence score (SS; Yang et al., CVPR 2020) and fixation edit distance (FED; Mondal et al., CVPR 2023) on the device
(csrc/seqscore.hip): the fixations of a group (all human fixations of an image) are clustered by flat-kernel mean shift
(Comaniciu & Meer 2002), a scanpath becomes the string of its fixations' cluster labels, SS = the Needleman-Wunsch score of two strings
with the 0/1 similarity divided by the longer length (gap 0: LCS / max(n, m)), FED = their Levenshtein distance.  Everything is float64
and bit-exact against the plain-loop checker tests/seqscore_ref.py.  The bandwidth has no default: it is the cluster radius in the
pixels of the fixations' frame and belongs to the data.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from ... import hip
from ...hip import check

METRICS = ("SS", "FED")
MAX_FIXATIONS = 64          # = sp_scan_max_fixations() and
MAX_POINTS = 1024           # = sp_meanshift_max_points(), known here so that a refusal needs no library (held equal by the tests)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise hip.HipError("scanpaths_amd sequence scores run on a HIP device only (no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


# ---- argument checks: every refusal comes before the device or the library is touched ---------------------------------------------------
def _check_cluster_args(bandwidth, max_iter) -> Tuple[float, int]:
    h = float(bandwidth)
    if not (np.isfinite(h) and h > 0):
        raise ValueError(f"bandwidth {bandwidth!r}: a positive finite number (pixels of the fixations' frame)")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"max_iter {max_iter!r}: an integer >= 1")
    return h, int(max_iter)


def _check_sequence_args(metrics, gap) -> Tuple[Tuple[str, ...], float]:
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    unknown = [m for m in metrics if m not in METRICS]
    if unknown:
        raise ValueError(f"unknown sequence metric {unknown[0]!r}: one of {METRICS}")
    if len(set(metrics)) != len(metrics):
        raise ValueError(f"repeated sequence metric in {metrics}")
    if not metrics:
        raise ValueError("no sequence metric asked for")
    g = float(gap)
    if not (np.isfinite(g) and g <= 0):
        raise ValueError(f"gap {gap!r}: a finite number <= 0")
    return metrics, g + 0.0                                  # -0.0 -> 0.0


def _rows(seqs, what: str, limit: int):
    """list of [n, >= 2] arrays -> (rows float64 [total, ncol], ncol, counts int32)"""
    arrs = [np.asarray(a, dtype=np.float64) for a in seqs]
    arrs = [a.reshape(len(a), -1) if len(a) else np.zeros((0, a.shape[-1] if a.ndim == 2 else 2)) for a in arrs]
    ncol = max([a.shape[1] for a in arrs if a.shape[0]], default=2)
    if any(a.shape[1] != ncol and a.shape[0] > 0 for a in arrs) or ncol < 2:
        raise ValueError(f"{what}s need the same number (>= 2) of columns")
    counts = np.array([a.shape[0] for a in arrs], dtype=np.int32)
    if len(counts) and counts.max() > limit:
        raise ValueError(f"{what} of {counts.max()} fixations exceeds the kernel limit {limit}")
    cat = np.concatenate([a for a in arrs if a.shape[0]] or [np.zeros((0, ncol))], 0)
    return np.ascontiguousarray(cat), ncol, counts


def _starts(counts) -> np.ndarray:
    return np.cumsum(counts, dtype=np.int64) - counts


def _index(values, n: int, what: str) -> np.ndarray:
    v = np.asarray(values, dtype=np.int64)
    if v.size and (v.min() < 0 or v.max() >= n):
        raise ValueError(f"{what} index out of range: {n} to choose from, indices {v.min()} .. {v.max()}")
    return v


def _centres(clusters):
    """clusters[g]: a [K, 2] array of centres, or the (centres, weight, labels) of meanshift_clusters"""
    cs = [np.asarray(c[0] if isinstance(c, tuple) else c, dtype=np.float64).reshape(-1, 2) for c in clusters]
    counts = np.array([len(c) for c in cs], dtype=np.int32)
    if len(counts) and counts.max() > MAX_POINTS:
        raise ValueError(f"{counts.max()} centres in a group exceed the kernel limit {MAX_POINTS}")
    return np.ascontiguousarray(np.concatenate(cs or [np.zeros((0, 2))], 0)), counts


def _strings(strings):
    ss = [np.asarray(s, dtype=np.int64).reshape(-1) for s in strings]
    counts = np.array([len(s) for s in ss], dtype=np.int32)
    if len(counts) and counts.max() > MAX_FIXATIONS:
        raise ValueError(f"string of {counts.max()} labels exceeds the kernel limit {MAX_FIXATIONS}")
    cat = np.concatenate(ss or [np.zeros(0, dtype=np.int64)])
    if cat.size and (cat.min() < -1 or cat.max() > np.iinfo(np.int32).max):
        raise ValueError("labels are int32 values >= 0 (or -1: no cluster)")
    return cat.astype(np.int32), counts


# ---- the one engine: one upload, one launch per entry point, one copy back -----------------------------------------------------------------
def _upload(arrays: Dict[str, np.ndarray], dev):
    """the named host arrays in one buffer, each at a multiple of 8 bytes -> (the device buffer, {name: device address})"""
    parts, off, pos = [], {}, 0
    for name, a in arrays.items():
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        off[name] = pos
        pad = -len(b) % 8
        parts += [b, np.zeros(pad, dtype=np.uint8)]
        pos += len(b) + pad
    buf = torch.from_numpy(np.concatenate(parts + [np.zeros(8, dtype=np.uint8)])).to(dev)
    return buf, {name: buf.data_ptr() + o for name, o in off.items()}


class _Out:
    """the results of a call in one device buffer (one copy back); sections at multiples of 8 bytes"""

    def __init__(self, sections, dev):
        self.at, pos = {}, 0
        for name, (dtype, n) in sections.items():
            self.at[name] = (pos, np.dtype(dtype), n)
            pos += (np.dtype(dtype).itemsize * n + 7) // 8 * 8
        self.buf = torch.empty(pos + 8, dtype=torch.uint8, device=dev)

    def ptr(self, name):
        return self.buf.data_ptr() + self.at[name][0] if name in self.at else None

    def host(self):
        raw = self.buf.cpu().numpy()                          # synchronises: every buffer of the call outlives its launches
        return {name: raw[o:o + dt.itemsize * n].view(dt).copy() for name, (o, dt, n) in self.at.items()}


def _run(*, rows, ncol=2, gstart=None, gcount=None, bandwidth=None, max_iter=None, centres=None, ncentres=None,
         start=None, count=None, group=None, pairs=None, gap=0.0, metrics=(), want=()):
    """Whatever stages the arguments name, chained on the device; returns the host copy of every result section.
      clusters: mean shift of the groups (gstart, gcount) of rows when bandwidth is given, else the host's centres / ncentres;
      strings:  the labels of the scanpaths (start, count) of rows under the centres of group[s]; without group, rows ARE the labels;
      scores:   SS / FED (metrics) of pairs.
    want: "weight" / "point_labels" of the mean shift, which nothing downstream needs (NULL otherwise)."""
    dev = _device()
    L = hip.lib()
    if L.sp_scan_max_fixations() != MAX_FIXATIONS or L.sp_meanshift_max_points() != MAX_POINTS:
        raise hip.HipError(f"kernel limits {L.sp_scan_max_fixations()} / {L.sp_meanshift_max_points()}, this module expects "
                           f"{MAX_FIXATIONS} / {MAX_POINTS}")
    nrows = len(rows)
    up = {"rows": rows if nrows else np.zeros((1, ncol))}
    if bandwidth is not None:
        up.update(gstart=gstart, gcount=gcount)
    elif centres is not None:
        up.update(centres=centres if len(centres) else np.zeros((1, 2)), gstart=_starts(ncentres), ncentres=ncentres)
    if start is not None:
        up.update(start=start, count=count)
    if group is not None:
        up.update(group=group.astype(np.int32))
    if pairs is not None:
        up.update(pairs=pairs.astype(np.int32).reshape(-1))
    buf, at = _upload(up, dev)
    npairs = 0 if pairs is None else len(pairs)
    clustering, labelling = bandwidth is not None, group is not None
    sections = {}
    if clustering:                                            # centres and ncentres feed the next stage whether wanted or not
        sections.update(centres=(np.float64, 2 * max(nrows, 1)), ncentres=(np.int32, len(gcount)))
        if "weight" in want:
            sections["weight"] = (np.int32, max(nrows, 1))
        if "point_labels" in want:
            sections["point_labels"] = (np.int32, max(nrows, 1))
    if labelling:
        sections["labels"] = (np.int32, max(nrows, 1))
    for m in METRICS:
        if m in metrics:
            sections[m] = (np.float64, npairs)
    out = _Out(sections, dev)
    s = hip.stream()
    if clustering:
        check(L.sp_meanshift(at["rows"], ncol, at["gstart"], at["gcount"], len(gcount), bandwidth, max_iter, out.ptr("centres"),
                             out.ptr("ncentres"), out.ptr("weight"), out.ptr("point_labels"), s), "sp_meanshift")
    if labelling:
        c_p, n_p = (out.ptr("centres"), out.ptr("ncentres")) if clustering else (at["centres"], at["ncentres"])
        check(L.sp_scan_cluster_strings(at["rows"], ncol, at["start"], at["count"], at["group"], len(count), c_p, at["gstart"], n_p,
                                        out.ptr("labels"), s), "sp_scan_cluster_strings")
    if npairs:
        lab_p = out.ptr("labels") if labelling else at["rows"]
        check(L.sp_scan_sequence(lab_p, at["start"], at["count"], at["pairs"], npairs, gap, out.ptr("SS"), out.ptr("FED"), s),
              "sp_scan_sequence")
    host = out.host()
    del buf                                                   # the upload lived until the copy back had synchronised
    return host


# ---- public calls ---------------------------------------------------------------------------------------------------------------------------
def meanshift_clusters(groups_of_points, *, bandwidth, max_iter: int = 300) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Flat-kernel mean shift of every group of points ([n, >= 2] arrays; x and y are read) with every point as a seed -- sklearn's
    MeanShift(bandwidth=bandwidth, bin_seeding=False, cluster_all=True, max_iter=max_iter) restated with a fixed order of operations
    (DESIGN.md §17).  bandwidth (required): the radius of the flat kernel, in the units of the points.  Returns per group
    (centres float64 [K, 2], weight int32 [K] = points within the bandwidth of the centre's last step, labels int32 [n] = the nearest
    centre of every point, the lowest on ties), clusters ordered by weight, then x, then y, descending.  One upload, one launch and one
    copy back for all groups; a group of more than MAX_POINTS points is refused."""
    h, max_iter = _check_cluster_args(bandwidth, max_iter)
    rows, ncol, counts = _rows(groups_of_points, "group", MAX_POINTS)
    if len(rows) == 0:
        return [(np.zeros((0, 2)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)) for _ in counts]
    gstart = _starts(counts)
    res = _run(rows=rows, ncol=ncol, gstart=gstart, gcount=counts, bandwidth=h, max_iter=max_iter, want=("weight", "point_labels"))
    cen = res["centres"].reshape(-1, 2)
    out = []
    for g, (o, n) in enumerate(zip(gstart, counts)):
        K = int(res["ncentres"][g])
        if K < 0:
            raise hip.HipError(f"sp_meanshift refused group {g} of {n} points")
        out.append((cen[o:o + K].copy(), res["weight"][o:o + K].copy(), res["point_labels"][o:o + n].copy()))
    return out


def cluster_strings(scanpaths, groups, clusters) -> List[np.ndarray]:
    """scanpaths[s] ([n <= 64, >= 2] array) as the int32 string of its fixations' clusters under clusters[groups[s]] (a [K, 2] array
    of centres or an item of meanshift_clusters' result): the nearest centre, the lowest on ties; -1 under a group without centres."""
    rows, ncol, counts = _rows(scanpaths, "scanpath", MAX_FIXATIONS)
    centres, ncentres = _centres(clusters)
    group = _index(groups, len(ncentres), "group").reshape(-1)
    if len(group) != len(counts):
        raise ValueError("one group per scanpath is required")
    if len(rows) == 0:
        return [np.zeros(0, dtype=np.int32) for _ in counts]
    start = _starts(counts)
    lab = _run(rows=rows, ncol=ncol, centres=centres, ncentres=ncentres, start=start, count=counts, group=group)["labels"]
    return [lab[o:o + n].copy() for o, n in zip(start, counts)]


def sequence_scores_pairs(strings, pairs, metrics=METRICS, gap: float = 0.0) -> Dict[str, np.ndarray]:
    """strings: int sequences of at most 64 labels >= 0 (cluster labels from cluster_strings, or any other labelling of the fixations:
    with segmentation labels this is the semantic sequence score); pairs: int [npairs, 2] = (index of a, index of b).
      "SS":  F[n][m] / max(n, m) of the Needleman-Wunsch table F[i][j] = max(F[i-1][j-1] + (a[i-1] == b[j-1]), F[i-1][j] + gap,
             F[i][j-1] + gap) with borders gap * i (gap <= 0; gap 0: LCS / max(n, m)); NaN for two empty strings;
      "FED": the Levenshtein distance (unit costs).
    Both NaN for a pair that holds a label -1.  Returns {metric: float64 numpy [npairs]}; one upload, one launch, one copy back."""
    metrics, gap = _check_sequence_args(metrics, gap)
    cat, counts = _strings(strings)
    pr = _index(pairs, len(counts), "pair").reshape(-1, 2)
    if len(pr) == 0:
        return {m: np.zeros(0, dtype=np.float64) for m in metrics}
    res = _run(rows=cat, start=_starts(counts), count=counts, pairs=pr, gap=gap, metrics=metrics)
    return {m: res[m] for m in metrics}


def _scores_under_centres(human, simulated, centres, metrics, gap):
    metrics, gap = _check_sequence_args(metrics, gap)
    rows, ncol, counts = _rows([human, simulated], "scanpath", MAX_FIXATIONS)
    cen, ncen = _centres([centres])
    return _run(rows=rows, ncol=ncol, centres=cen, ncentres=ncen, start=_starts(counts), count=counts, group=np.zeros(2, dtype=np.int64),
                pairs=np.array([[0, 1]]), gap=gap, metrics=metrics)


def sequence_score(human, simulated, centres, gap: float = 0.0) -> float:
    """SS of two scanpaths under the cluster centres [K, 2] of their image (meanshift_clusters of all its human fixations)"""
    return float(_scores_under_centres(human, simulated, centres, ("SS",), gap)["SS"][0])


def fixation_edit_distance(human, simulated, centres) -> float:
    """FED of two scanpaths under the cluster centres [K, 2] of their image"""
    return float(_scores_under_centres(human, simulated, centres, ("FED",), 0.0)["FED"][0])


def keyed_sequence_scores(scanpaths, path_group, human_group, pairs, num_groups: int, *, bandwidth, metrics=METRICS, gap: float = 0.0,
                          max_iter: int = 300) -> Dict[str, np.ndarray]:
    """The whole chain in one batch (what utils.evaluation's keyed calls run): the fixations of the scanpaths with human_group[i] = g
    >= 0 are the points of cluster group g (human_group[i] < 0: a prediction, it adds no points); scanpath i is written as a string
    under the clusters of path_group[i]; pairs[p] = (index of a, index of b).  One upload (the points are the human scanpaths' own
    rows), one launch per entry point, one copy back.  Returns {metric: float64 [npairs]}."""
    h, max_iter = _check_cluster_args(bandwidth, max_iter)
    metrics, gap = _check_sequence_args(metrics, gap)
    path_group = _index(path_group, num_groups, "group").reshape(-1)
    human_group = np.asarray(human_group, dtype=np.int64).reshape(-1)
    if not (len(path_group) == len(human_group) == len(scanpaths)):
        raise ValueError("one group per scanpath is required")
    if human_group.size and human_group.max() >= num_groups:
        raise ValueError(f"group index out of range: {num_groups} groups, index {human_group.max()}")
    pr = _index(pairs, len(scanpaths), "pair").reshape(-1, 2)
    # the human scanpaths first, sorted by group, so that the fixations of a group are consecutive rows
    humans = np.flatnonzero(human_group >= 0)
    humans = humans[np.argsort(human_group[humans], kind="stable")]
    order = np.concatenate([humans, np.flatnonzero(human_group < 0)]).astype(np.int64)
    rows, ncol, counts = _rows([scanpaths[i] for i in order], "scanpath", MAX_FIXATIONS)
    gcount = np.bincount(human_group[humans], weights=counts[:len(humans)], minlength=num_groups).astype(np.int32)
    if len(gcount) and gcount.max() > MAX_POINTS:
        raise ValueError(f"group of {gcount.max()} fixations exceeds the kernel limit {MAX_POINTS}")
    if len(pr) == 0:
        return {m: np.zeros(0, dtype=np.float64) for m in metrics}
    place = np.empty(len(order), dtype=np.int64)
    place[order] = np.arange(len(order))
    res = _run(rows=rows, ncol=ncol, gstart=_starts(gcount), gcount=gcount, bandwidth=h, max_iter=max_iter, start=_starts(counts),
               count=counts, group=path_group[order], pairs=place[pr], gap=gap, metrics=metrics)
    return {m: res[m] for m in metrics}
