"""Host restatement of csrc/scanboot.hip -- TEST INFRASTRUCTURE ONLY, numpy and plain Python, no torch, no kernel of the package.

Every sum is taken in the kernel's own stated order, so the GPU tests compare bit for bit:
  * draws                 -- the cluster index of every (replicate, draw), through sampling_ref.philox4x32_10;
  * cluster_sums          -- N, D per cluster in ascending key order from 0.0;
  * replicate_sums        -- lane l adds draws l, l + 64, .. from 0.0, the 64 partial sums combine by the xor butterfly 32 .. 1;
  * contrasts             -- (R[i] - R[j]) / (R[k] - R[l]) with the -1 rules;
  * resample / estimate   -- the two outputs of sp_boot_resample;
  * summary               -- the counts, the two-pass mean and standard deviation and the order-statistic quantiles of sp_boot_summarise;
  * replicate_sums_fsum   -- the same sums free of any order (math.fsum: the correctly rounded sum), to hold the ordered ones to the
                             textbook error bound; exact_ratios does so from the keys themselves, without cluster sums in between;
  * bootstrap             -- all of it behind bootstrap_ratio's interface."""
from __future__ import annotations

import math

import numpy as np

from sampling_ref import philox4x32_10

_ERR = dict(invalid="ignore", divide="ignore", over="ignore")


def draws(B, C, seed, b0=0):
    """int64 [B, C]: the cluster of draw j of replicate b0 + b: word j & 3 of the Philox block with key (seed lo, seed hi) and counter
    (b, j >> 2, 0, 1); index (word * C) >> 32"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nblocks = (C + 3) // 4
    b = (np.arange(B, dtype=np.uint64) + np.uint64(b0))[:, None]
    blk = np.arange(nblocks, dtype=np.uint64)[None, :]
    words = philox4x32_10((b, blk, np.uint64(0), np.uint64(1)), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack([x.astype(np.uint64) for x in words], -1).reshape(B, nblocks * 4)[:, :C]
    return ((w * np.uint64(C)) >> np.uint64(32)).astype(np.int64)


def cluster_sums(num, den, labels, C):
    """N, D float64 [C, M]: the rows of a cluster added in ascending key order from 0.0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    N, D = np.zeros((C, num.shape[1])), np.zeros((C, num.shape[1]))
    with np.errstate(**_ERR):
        for g, c in enumerate(labels):
            N[c] = N[c] + num[g]
            D[c] = D[c] + den[g]
    return N, D


def _butterfly(v):
    """v [..., 64, M]: the wave's xor butterfly over the lane axis; every lane ends with the same total, lane 0's is returned"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o, :]
    return v[..., 0, :]


def replicate_sums(T, idx):
    """T [C, M], idx int64 [B, C] -> [B, M]: sum_j T[idx[b, j]] in the kernel's order"""
    B, C = idx.shape
    rows = -(-C // 64)
    pad = np.full((B, rows * 64), -1, dtype=np.int64)
    pad[:, :C] = idx
    pad = pad.reshape(B, rows, 64)
    Tz = np.concatenate([T, np.zeros((1, T.shape[1]))], 0)             # row -1: a lane without a draw adds nothing (0.0)
    with np.errstate(**_ERR):
        acc = np.zeros((B, 64, T.shape[1]))
        for r in range(rows):
            live = (pad[:, r, :] >= 0)[..., None]
            acc = np.where(live, acc + Tz[pad[:, r, :]], acc)
        return _butterfly(acc)


def replicate_sums_fsum(T, idx):
    """the same sums, correctly rounded whatever the order (finite inputs)"""
    return np.array([[math.fsum(T[row, m]) for m in range(T.shape[1])] for row in idx], dtype=np.float64).reshape(len(idx), T.shape[1])


def exact_ratios(num, den, labels, idx):
    """[B, M]: fsum of every key's num over the drawn clusters' members / the same of den -- no cluster sums in between, no order"""
    members = [np.flatnonzero(np.asarray(labels) == c) for c in range(int(np.max(labels)) + 1)]
    out = np.empty((len(idx), num.shape[1]))
    for b, row in enumerate(idx):
        g = np.concatenate([members[c] for c in row])
        out[b] = [math.fsum(num[g, m]) / math.fsum(den[g, m]) for m in range(num.shape[1])]
    return out


def contrasts(R, con):
    """R [B, M], con int [S, 4] -> [S, B]"""
    out = np.empty((len(con), len(R)))
    with np.errstate(**_ERR):
        for s, (i, j, k, l) in enumerate(np.asarray(con, dtype=np.int64)):
            v = R[:, i].copy()
            if j != -1:
                v = v - R[:, j]
            if k != -1:
                u = R[:, k].copy()
                if l != -1:
                    u = u - R[:, l]
                v = v / u
            out[s] = v
    return out


def _ratio(N, D, idx, con, sums=replicate_sums):
    with np.errstate(**_ERR):
        return contrasts(sums(N, idx) / sums(D, idx), con)


def resample(N, D, con, B, seed, sums=replicate_sums):
    """stat float64 [S, B]"""
    return _ratio(N, D, draws(B, len(N), seed), con, sums)


def estimate(N, D, con):
    """the point estimate [S]: every cluster once, cluster c at position c of the same order"""
    return _ratio(N, D, np.arange(len(N), dtype=np.int64)[None, :], con)[:, 0]


def _block_sum(x):
    """x [B] (invalid entries already 0.0): thread t adds t, t + 256, .. from 0.0; butterfly per wave; ((w0 + w1) + w2) + w3"""
    rows = -(-len(x) // 256)
    pad = np.zeros(rows * 256)
    pad[:len(x)] = x
    with np.errstate(**_ERR):
        acc = np.zeros(256)
        for r in pad.reshape(rows, 256):
            acc = acc + r
        w = _butterfly(acc.reshape(4, 64, 1))[:, 0]
        return ((w[0] + w[1]) + w[2]) + w[3]


def quantile_rank(q, n):
    return min(max(math.ceil(float(q) * float(n)) - 1, 0), n - 1)


def summary(stat, q):
    """stat [S, B] -> dict of mean, se [S], quantiles [S, Q], n_valid, n_le0, n_ge0 int32 [S]"""
    S, B = stat.shape
    nan = float("nan")
    res = {"mean": np.full(S, nan), "se": np.full(S, nan), "quantiles": np.full((S, len(q)), nan),
           "n_valid": np.zeros(S, np.int32), "n_le0": np.zeros(S, np.int32), "n_ge0": np.zeros(S, np.int32)}
    with np.errstate(**_ERR):
        for s, v in enumerate(stat):
            ok = ~np.isnan(v)
            n = int(ok.sum())
            res["n_valid"][s], res["n_le0"][s], res["n_ge0"][s] = n, int((ok & (v <= 0)).sum()), int((ok & (v >= 0)).sum())
            if n == 0:
                continue
            mean = _block_sum(np.where(ok, v, 0.0)) / float(n)
            res["mean"][s] = mean
            d = v - mean
            if n > 1:
                res["se"][s] = np.sqrt(_block_sum(np.where(ok, d * d, 0.0)) / float(n - 1))
            ordered = np.sort(v[ok], kind="stable")                      # the values alone: ties are equal values, +-inf sort exactly
            for k, qk in enumerate(q):
                res["quantiles"][s, k] = ordered[quantile_rank(qk, n)]
    return res


def bootstrap(num, den, clusters=None, con=None, *, replicates, seed, quantiles=(0.025, 0.975), sums=replicate_sums):
    """bootstrap_ratio on the host: its dict plus "replicates" [S, B]"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    if num.ndim == 1:
        num, den = num[:, None], den[:, None]
    G, M = num.shape
    labels = np.arange(G) if clusters is None else np.asarray(clusters, dtype=np.int64)
    C = int(labels.max()) + 1
    if con is None:
        con = [(m, -1, -1, -1) for m in range(M)]
    N, D = cluster_sums(num, den, labels, C)
    stat = resample(N, D, con, replicates, seed, sums)
    res = summary(stat, np.asarray(quantiles, dtype=np.float64).reshape(-1))
    res["estimate"] = estimate(N, D, con)
    res["replicates"] = stat
    return res
