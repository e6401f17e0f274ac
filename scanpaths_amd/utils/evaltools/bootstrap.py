"""Cluster bootstrap on the device (csrc/scanboot.hip): standard errors, percentile intervals and paired comparisons for
every keyed score table of utils/evaluation.py (Efron & Tibshirani 1993; the cluster bootstrap of Field & Welsh 2007 and Cameron,
Gelbach & Miller 2008).

    num, den, keys = table_columns(per_key, ["DTW", "DTW_best"])                   # the nanmean over keys as a ratio of sums
    res = bootstrap_ratio(num, den, clusters, contrasts, replicates=10000, seed=1)
    # {"estimate" [S], "mean" [S], "se" [S], "quantiles" [S, Q], "n_valid" [S], "n_le0" [S], "n_ge0" [S]}

THE STATISTIC.  For columns m the caller gives num [G, M] and den [G, M] (float64) and a dense cluster label in [0, C) per key -- the
image of the key: AiR has several questions per image and every dataset several subjects, so keys are not independent and the
resampling unit is the image.  N[c][m] / D[c][m] are the sums of num / den over the keys of cluster c in ascending key order.  A
replicate b draws C clusters with replacement and has the column values R[b][m] = (sum_j N[i(b, j)][m]) / (sum_j D[i(b, j)][m]); IEEE
division, 0 / 0 = NaN, and a NaN replicate is invalid for whatever it enters.  The nanmean over keys is num = the value (0 where NaN), den
= 1 (0 where NaN): table_columns.  The pooled mean of the likelihood family is num = the key's sum, den = the key's count, for a caller
who holds them.  A -inf value is a score and goes through the sums by IEEE rules.
The reported statistics are contrasts (i, j, k, l) of columns: stat[b] = (R[b][i] - R[b][j]) / (R[b][k] - R[b][l]); j = -1 subtracts
nothing, k = -1 means no division, l = -1 subtracts nothing in the denominator.  A plain score is (i, -1, -1, -1), a paired difference
(a, b, -1, -1), a ratio of differences (i, -1, k, l), a relative improvement (a, b, b, -1).  ALL COLUMNS OF A CALL SHARE THE DRAWS:
that is what makes a difference paired.
THE DRAWS.  Draw j of replicate b is word j & 3 of the Philox4x32-10 block with key (seed & 0xffffffff, seed >> 32) and counter (b, j >>
2, 0, 1); the cluster is (word * C) >> 32.  That rule selects a cluster with a probability that is off by at most C / 2^32 per cluster
(2^32 is not a multiple of C): relative to 1 / C that is 2.3e-7 at C = 1000.  C above 2^24 is refused, which keeps it below 2^-8.
THE SUMMARY per statistic over its valid (non-NaN) replicates: "n_valid"; "n_le0" / "n_ge0", how many are <= 0 / >= 0; "mean"; "se", the
standard deviation with ddof = 1 (NaN for n_valid < 2); "quantiles", order statistics without interpolation -- the replicate of rank
min(max(ceil(q * n_valid) - 1, 0), n_valid - 1) in ascending order --, so +-inf replicates stay exact; NaN without a valid replicate.
"estimate" is the same contrast on the data itself (every cluster once).  Every sum has a fixed order (csrc/scanboot.hip), so a call is
reproducible to the bit and tests/bootstrap_ref.py restates it in numpy.
One upload, one launch for the cluster sums, one per column chunk, two for the summary, and one copy back of the summary per call; the replicates
stay on the device (return_replicates=True hands the tensor out, uncopied).  The kernel holds MAX_COLUMNS columns per launch; wider
tables are cut into chunks that each hold all columns of their contrasts (column_chunks) and run with the same seed, hence the same
draws.  There is no CPU path.  table_columns, key_clusters and column_chunks are pure numpy."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr
from . import _batch

MAX_COLUMNS = 32            # = sp_boot_max_columns(), known here so that a refusal needs no library (held equal by the tests)
MAX_CLUSTERS = 1 << 24


def _device() -> torch.device:
    return _batch.device("the bootstrap runs")


# ---- argument checks: every refusal comes before the device or the library is touched ---------------------------------------------------
def _integers(values, what) -> np.ndarray:
    """values as int64 if every one of them is an integer (whatever the dtype), or ValueError"""
    a = np.asarray(values)
    if a.dtype.kind in "iu":
        return a.astype(np.int64)
    if a.dtype.kind == "f" and np.isfinite(a).all() and (a == np.floor(a)).all():
        return a.astype(np.int64)
    raise ValueError(f"{what} must be integers")


def _integer(value, what, lo, hi) -> int:
    if value is None or isinstance(value, bool) or not np.isscalar(value) or int(value) != value or not lo <= int(value) <= hi:
        raise ValueError(f"{what} {value!r}: an integer in [{lo}, {hi}] is required")
    return int(value)


def _check_table(num, den) -> Tuple[np.ndarray, np.ndarray]:
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    if num.shape != den.shape:
        raise ValueError(f"num {num.shape} and den {den.shape}: equal shapes are required")
    if num.ndim == 1:
        num, den = num[:, None], den[:, None]
    if num.ndim != 2 or num.shape[1] < 1:
        raise ValueError(f"num and den are [G, M] arrays (or [G] for one column), got shape {num.shape}")
    if num.shape[0] < 1:
        raise ValueError("G = 0: a table without keys has no bootstrap")
    return np.ascontiguousarray(num), np.ascontiguousarray(den)


def _check_clusters(clusters, G) -> Tuple[np.ndarray, int]:
    if clusters is None:
        labels = np.arange(G, dtype=np.int64)
    else:
        labels = _integers(clusters, "cluster labels").reshape(-1)
        if len(labels) != G:
            raise ValueError(f"one cluster label per key is required: {len(labels)} labels, {G} keys")
        if labels.min() < 0:
            raise ValueError(f"cluster labels must not be negative, got {labels.min()}")
    C = int(labels.max()) + 1
    if C > MAX_CLUSTERS:
        raise ValueError(f"{C} clusters exceed the limit {MAX_CLUSTERS} (2^24) of the draw rule")
    if clusters is not None:
        unused = np.flatnonzero(np.bincount(labels, minlength=C) == 0)
        if len(unused):
            raise ValueError(f"cluster labels must be dense in [0, {C}): label {unused[0]} is unused (an empty cluster would be drawn)")
    return labels, C


def _check_contrasts(contrasts, M) -> np.ndarray:
    if contrasts is None:
        c = np.full((M, 4), -1, dtype=np.int64)
        c[:, 0] = np.arange(M)
        return c.astype(np.int32)
    c = _integers(contrasts, "contrast indices")
    if c.ndim != 2 or c.shape[1] != 4 or c.shape[0] < 1:
        raise ValueError(f"contrasts is an [S, 4] array of (i, j, k, l) with S >= 1, got shape {c.shape}")
    if c[:, 0].min() < 0 or c.min() < -1 or c.max() >= M:
        raise ValueError(f"contrast index out of range: {M} columns, i in [0, {M}) and j, k, l in [-1, {M}), got {c.min()} .. {c.max()}")
    return c.astype(np.int32)


def _check_quantiles(quantiles) -> np.ndarray:
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    if not ((q >= 0) & (q <= 1)).all():                      # NaN fails both comparisons
        raise ValueError(f"quantiles {q.tolist()}: every q must lie in [0, 1]")
    return q


def column_chunks(contrasts, limit: int = MAX_COLUMNS) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The launches of a contrast table [S, 4]: a list of (columns int64 [Mc <= limit], contrasts int32 [Sc, 4] with indices into
    columns), the contrasts in their order.  A chunk is closed when the next contrast's columns no longer fit; a column that several
    chunks need is simply given to each of them, so every contrast finds all of its columns in its own chunk."""
    out, cols, where, rows = [], [], {}, []

    def close():
        if rows:
            out.append((np.array(cols, dtype=np.int64), np.array(rows, dtype=np.int32).reshape(-1, 4)))

    for c in np.asarray(contrasts, dtype=np.int64).reshape(-1, 4):
        new = [int(m) for m in dict.fromkeys(c.tolist()) if m >= 0 and int(m) not in where]
        if len(cols) + len(new) > limit:
            close()
            cols, where, rows = [], {}, []
            new = [int(m) for m in dict.fromkeys(c.tolist()) if m >= 0]
        for m in new:
            where[m] = len(cols)
            cols.append(m)
        rows.append([where[int(m)] if m >= 0 else -1 for m in c])
    close()
    return out


# ---- the device call -------------------------------------------------------------------------------------------------------------------------
def bootstrap_ratio(num, den, clusters=None, contrasts=None, *, replicates, seed, quantiles=(0.025, 0.975),
                    return_replicates=False) -> Dict[str, object]:
    """num, den: float64 [G, M] (or [G]: one column); clusters: int [G], dense labels in [0, C), C <= 2^24 (None: every key its own
    cluster); contrasts: int [S, 4] of (i, j, k, l) (None: one plain contrast per column); replicates >= 1 and seed in [0, 2^64) have no
    defaults; quantiles: any number of q in [0, 1].
    Returns {"estimate", "mean", "se" float64 [S], "quantiles" float64 [S, Q], "n_valid", "n_le0", "n_ge0" int32 [S]} and, with
    return_replicates, "replicates": the float64 [S, B] tensor on the device, not copied back (module docstring)."""
    num, den = _check_table(num, den)
    G, M = num.shape
    labels, C = _check_clusters(clusters, G)
    con = _check_contrasts(contrasts, M)
    B = _integer(replicates, "replicates", 1, 2 ** 31 - 2)
    seed = _integer(seed, "seed", 0, 2 ** 64 - 1)
    q = _check_quantiles(quantiles)
    S, Q = len(con), len(q)
    chunks = column_chunks(con, MAX_COLUMNS)
    cols = np.concatenate([c for c, _ in chunks])
    W = len(cols)                                                    # the width of the uploaded table: every chunk's columns in a row
    order = np.argsort(labels, kind="stable")                        # keys by cluster, ascending key index inside a cluster
    count = np.bincount(labels, minlength=C).astype(np.int32)
    dev = _device()
    L = hip.lib()
    if L.sp_boot_max_columns() != MAX_COLUMNS:
        raise hip.HipError(f"sp_boot_max_columns() = {L.sp_boot_max_columns()}, this module expects {MAX_COLUMNS}")
    buf, at = _batch.upload({"num": num[order][:, cols], "den": den[order][:, cols], "starts": _batch.starts(count), "counts": count,
                             "contrast": np.concatenate([c for _, c in chunks]), "q": q}, dev)
    sums = torch.empty(2 * C * W, dtype=torch.float64, device=dev)
    stat = torch.empty((S, B), dtype=torch.float64, device=dev)
    out = _batch.Out({"estimate": (np.float64, S), "mean": (np.float64, S), "se": (np.float64, S), "quantiles": (np.float64, S * Q),
                      "n_valid": (np.int32, S), "n_le0": (np.int32, S), "n_ge0": (np.int32, S)}, dev)
    stream = hip.stream()
    pN, pD = ptr(sums), ptr(sums) + 8 * C * W
    check(L.sp_boot_cluster_sums(at["num"], at["den"], at["starts"], at["counts"], G, C, W, pN, pD, stream), "sp_boot_cluster_sums")
    c0 = s0 = 0
    for columns, local in chunks:
        check(L.sp_boot_resample(pN + 8 * c0, pD + 8 * c0, C, len(columns), W, at["contrast"] + 16 * s0, len(local), B, seed,
                                 ptr(stat) + 8 * s0 * B, out.ptr("estimate") + 8 * s0, stream), "sp_boot_resample")
        c0, s0 = c0 + len(columns), s0 + len(local)
    check(L.sp_boot_summarise(ptr(stat), S, B, at["q"], Q, out.ptr("mean"), out.ptr("se"), out.ptr("quantiles"), out.ptr("n_valid"),
                              out.ptr("n_le0"), out.ptr("n_ge0"), stream), "sp_boot_summarise")
    res: Dict[str, object] = out.host()
    res["quantiles"] = res["quantiles"].reshape(S, Q)
    if return_replicates:
        res["replicates"] = stat
    return res


# ---- pure numpy: from keyed score tables to columns ---------------------------------------------------------------------------------------
def table_columns(per_key, names: Sequence[str]) -> Tuple[np.ndarray, np.ndarray, list]:
    """per_key: the second result of a keyed evaluation (a dict with "keys" and float64 [G] entries), or a sequence of them from several
    batches, which is concatenated -- a key that appears in two batches contributes two rows (of one cluster: key_clusters).
    Returns (num [G, len(names)], den, keys): num = the value and den = 1, both 0 where the value is NaN, so that sum num / sum den is
    the nanmean over keys."""
    tables = [per_key] if isinstance(per_key, dict) else list(per_key)
    names = list(names)
    if not tables:
        raise ValueError("at least one per_key table is required")
    keys, blocks = [], []
    for t in tables:
        k = list(t["keys"])
        missing = [n for n in names if n not in t]
        if missing:
            raise ValueError(f"the table holds no entry {missing[0]!r}")
        cols = [np.asarray(t[n], dtype=np.float64).reshape(-1) for n in names]
        if any(len(c) != len(k) for c in cols):
            raise ValueError(f"every entry needs one value per key: {len(k)} keys, entries of {sorted(set(map(len, cols)))} values")
        keys += k
        blocks.append(np.stack(cols, 1) if cols else np.zeros((len(k), 0)))
    value = np.concatenate(blocks, 0)
    nan = np.isnan(value)
    return np.where(nan, 0.0, value), np.where(nan, 0.0, 1.0), keys


def key_clusters(keys, cluster_keys=None) -> np.ndarray:
    """int64 [G]: a dense cluster label per key, in first-appearance order.  cluster_keys None: the key is its own cluster (the same key
    in two batches is one cluster); a mapping: cluster_keys[key] is the key's image; else a sequence aligned with keys."""
    keys = list(keys)
    if cluster_keys is None:
        images = keys
    elif hasattr(cluster_keys, "keys") and hasattr(cluster_keys, "__getitem__"):
        missing = [k for k in keys if k not in cluster_keys]
        if missing:
            raise ValueError(f"cluster_keys holds no image for key {missing[0]!r} ({len(missing)} in all)")
        images = [cluster_keys[k] for k in keys]
    else:
        images = list(cluster_keys)
        if len(images) != len(keys):
            raise ValueError(f"one cluster key per key is required: {len(images)} cluster keys, {len(keys)} keys")
    index: dict = {}
    return np.array([index.setdefault(im, len(index)) for im in images], dtype=np.int64)
