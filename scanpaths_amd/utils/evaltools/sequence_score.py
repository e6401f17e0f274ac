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
from . import _batch
from ._batch import MAX_FIXATIONS, check_index, check_pairs, pack, starts

METRICS = ("SS", "FED")
MAX_POINTS = 1024           # = sp_meanshift_max_points(), known here so that a refusal needs no library (held equal by the tests)


def _device() -> torch.device:
    return _batch.device("sequence scores run")


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
def _run(*, rows, ncol=2, gstart=None, gcount=None, bandwidth=None, max_iter=None, centres=None, ncentres=None,
         start=None, count=None, group=None, pairs=None, gap=0.0, metrics=(), want=()):
    """Whatever stages the arguments name, chained on the device; returns the host copy of every result section.
      clusters: mean shift of the groups (gstart, gcount) of rows when bandwidth is given, else the host's centres / ncentres;
      strings:  the labels of the scanpaths (start, count) of rows under the centres of group[s]; without group, rows ARE the labels;
      scores:   SS / FED (metrics) of pairs.
    want: "weight" / "point_labels" of the mean shift, which nothing downstream needs (NULL otherwise)."""
    dev = _device()
    L = hip.lib()
    _batch.check_limits(L, MAX_POINTS)
    nrows = len(rows)
    up = {"rows": rows}
    if bandwidth is not None:
        up.update(gstart=gstart, gcount=gcount)
    elif centres is not None:
        up.update(centres=centres, gstart=starts(ncentres), ncentres=ncentres)
    if start is not None:
        up.update(start=start, count=count)
    if group is not None:
        up.update(group=group.astype(np.int32))
    if pairs is not None:
        up.update(pairs=pairs.astype(np.int32))
    buf, at = _batch.upload(up, dev)
    npairs = 0 if pairs is None else len(pairs)
    clustering, labelling = bandwidth is not None, group is not None
    sections = {}
    if clustering:                                            # centres and ncentres feed the next stage whether wanted or not
        sections.update(centres=(np.float64, 2 * nrows), ncentres=(np.int32, len(gcount)))
        sections.update({k: (np.int32, nrows) for k in ("weight", "point_labels") if k in want})
    if labelling:
        sections["labels"] = (np.int32, nrows)
    sections.update({m: (np.float64, npairs) for m in METRICS if m in metrics})
    out = _batch.Out(sections, dev)
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
    return out.host()


# ---- public calls ---------------------------------------------------------------------------------------------------------------------------
def meanshift_clusters(groups_of_points, *, bandwidth, max_iter: int = 300) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Flat-kernel mean shift of every group of points ([n, >= 2] arrays; x and y are read) with every point as a seed -- sklearn's
    MeanShift(bandwidth=bandwidth, bin_seeding=False, cluster_all=True, max_iter=max_iter) restated with a fixed order of operations
    (DESIGN.md §17).  bandwidth (required): the radius of the flat kernel, in the units of the points.  Returns per group
    (centres float64 [K, 2], weight int32 [K] = points within the bandwidth of the centre's last step, labels int32 [n] = the nearest
    centre of every point, the lowest on ties), clusters ordered by weight, then x, then y, descending.  One upload, one launch and one
    copy back for all groups; a group of more than MAX_POINTS points is refused."""
    h, max_iter = _check_cluster_args(bandwidth, max_iter)
    rows, ncol, counts, gstart = pack(groups_of_points, min_cols=2, what="group", limit=MAX_POINTS)
    if len(rows) == 0:
        return [(np.zeros((0, 2)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)) for _ in counts]
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
    rows, ncol, counts, start = pack(scanpaths, min_cols=2)
    centres, ncentres = _centres(clusters)
    group = check_index(groups, len(ncentres), "group").reshape(-1)
    if len(group) != len(counts):
        raise ValueError("one group per scanpath is required")
    if len(rows) == 0:
        return [np.zeros(0, dtype=np.int32) for _ in counts]
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
    pr = check_pairs(pairs, len(counts))
    if len(pr) == 0:
        return {m: np.zeros(0, dtype=np.float64) for m in metrics}
    res = _run(rows=cat, start=starts(counts), count=counts, pairs=pr, gap=gap, metrics=metrics)
    return {m: res[m] for m in metrics}


def _scores_under_centres(human, simulated, centres, metrics, gap):
    metrics, gap = _check_sequence_args(metrics, gap)
    rows, ncol, counts, start = pack([human, simulated], min_cols=2)
    cen, ncen = _centres([centres])
    return _run(rows=rows, ncol=ncol, centres=cen, ncentres=ncen, start=start, count=counts, group=np.zeros(2, dtype=np.int64),
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
    path_group = check_index(path_group, num_groups, "group").reshape(-1)
    human_group = np.asarray(human_group, dtype=np.int64).reshape(-1)
    if not (len(path_group) == len(human_group) == len(scanpaths)):
        raise ValueError("one group per scanpath is required")
    if human_group.size and human_group.max() >= num_groups:
        raise ValueError(f"group index out of range: {num_groups} groups, index {human_group.max()}")
    pr = check_pairs(pairs, len(scanpaths))
    # the human scanpaths first, sorted by group, so that the fixations of a group are consecutive rows
    humans = np.flatnonzero(human_group >= 0)
    humans = humans[np.argsort(human_group[humans], kind="stable")]
    order = np.concatenate([humans, np.flatnonzero(human_group < 0)]).astype(np.int64)
    rows, ncol, counts, start = pack([scanpaths[i] for i in order], min_cols=2)
    gcount = np.bincount(human_group[humans], weights=counts[:len(humans)], minlength=num_groups).astype(np.int32)
    if len(gcount) and gcount.max() > MAX_POINTS:
        raise ValueError(f"group of {gcount.max()} fixations exceeds the kernel limit {MAX_POINTS}")
    if len(pr) == 0:
        return {m: np.zeros(0, dtype=np.float64) for m in metrics}
    place = np.empty(len(order), dtype=np.int64)
    place[order] = np.arange(len(order))
    res = _run(rows=rows, ncol=ncol, gstart=starts(gcount), gcount=gcount, bandwidth=h, max_iter=max_iter, start=start, count=counts,
               group=path_group[order], pairs=place[pr], gap=gap, metrics=metrics)
    return {m: res[m] for m in metrics}
