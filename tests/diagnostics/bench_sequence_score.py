"""Sequence score and fixation edit distance of a validation call: sequence_score_evaluation on the device against the Python checker
(tests/seqscore_ref.py, plain loops -- the shape of the published nw_matching code) and, where it is installed, sklearn's MeanShift once
per key (what the published evaluation clusters with) on one core.  Workload: that of tests/diagnostics/bench_scanpath_distances.py --
500 keys, 3-10 human and 20 predicted scanpaths per key, 3-16 fixations each in a 320x240 frame; bandwidth 25.
    python tests/diagnostics/bench_sequence_score.py [--keys 500] [--host-keys 25] [--reps 5] [--out profiles/bench_sequence_score.json]
The device time is a host clock around the whole keyed call (packing, the one upload, three launches, the one copy back, which
synchronises, and the per-key grouping on the host); the three batched calls alone (meanshift_clusters, cluster_strings,
sequence_scores_pairs) are timed as well.  One warm-up call comes first.  The host time is the checker over a seeded random subset of
--host-keys keys (clustering, strings and all their pairs), scaled to all keys (0: all of them).  Prints one JSON line and writes it
to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workload(keys, g):
    def scanpath():
        n = int(g.integers(3, 17))
        return np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.08, 0.6, n)], 1)

    gt, gt_k, pr, pr_k = [], [], [], []
    for q in range(keys):
        nh = int(g.integers(3, 11))
        gt += [scanpath() for _ in range(nh)]
        gt_k += [q] * nh
        pr += [scanpath() for _ in range(20)]
        pr_k += [q] * 20
    return gt, gt_k, pr, pr_k


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=500)
    ap.add_argument("--host-keys", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bandwidth", type=float, default=25.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sequence_score.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sequence_score needs a HIP device: a time taken elsewhere says nothing")
    import seqscore_ref as R
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import sequence_score as S
    h = a.bandwidth
    gt, gt_k, pr, pr_k = workload(a.keys, np.random.Generator(np.random.PCG64(0)))
    paths = [p[:, :2] for p in gt] + [p[:, :2] for p in pr]
    humans = {}
    for i, k in enumerate(gt_k):
        humans.setdefault(k, []).append(i)
    pooled = [np.concatenate([paths[i] for i in humans[q]], 0) for q in range(a.keys)]
    pairs = np.array([(i, len(gt) + j) for j, k in enumerate(pr_k) for i in humans[k]], dtype=np.int64)
    pair_key = np.array([k for k in pr_k for _ in humans[k]], dtype=np.int64)

    E.sequence_score_evaluation(gt, pr, gt_k, pr_k, bandwidth=h)     # warm-up: code objects, allocator
    (means, _), t_call = timed(lambda: E.sequence_score_evaluation(gt, pr, gt_k, pr_k, bandwidth=h), a.reps)
    clusters, t_ms = timed(lambda: S.meanshift_clusters(pooled, bandwidth=h), a.reps)
    strings, t_str = timed(lambda: S.cluster_strings(paths, gt_k + pr_k, clusters), a.reps)
    dev, t_seq = timed(lambda: S.sequence_scores_pairs(strings, pairs), a.reps)

    g = np.random.Generator(np.random.PCG64(1))
    nk = a.keys if a.host_keys <= 0 else min(a.host_keys, a.keys)
    sub = np.sort(g.choice(a.keys, nk, replace=False)) if nk < a.keys else np.arange(a.keys)
    t0 = time.perf_counter()
    host_clusters = {q: R.meanshift_loops(pooled[q], h) for q in sub}
    t_host_ms = time.perf_counter() - t0
    t0 = time.perf_counter()
    sel = np.flatnonzero(np.isin(pair_key, sub))
    host_strings = {i: R.labels_of(paths[i], host_clusters[(gt_k + pr_k)[i]][0]) for i in np.unique(pairs[sel])}
    host = {m: np.array([fn(host_strings[i], host_strings[j]) for i, j in pairs[sel]])
            for m, fn in (("SS", R.sequence_score), ("FED", R.fixation_edit_distance))}
    t_host_seq = time.perf_counter() - t0
    differ = {m: int((~((host[m] == dev[m][sel]) | (np.isnan(host[m]) & np.isnan(dev[m][sel])))).sum()) for m in ("SS", "FED")}
    differ["clusters"] = int(sum(not all(np.array_equal(x, y) for x, y in zip(host_clusters[q], clusters[q])) for q in sub))
    t_sk = None
    try:
        from sklearn.cluster import MeanShift
        t0 = time.perf_counter()
        for q in sub:
            MeanShift(bandwidth=h, bin_seeding=False, cluster_all=True).fit(pooled[q])
        t_sk = time.perf_counter() - t0
    except ImportError:
        pass
    scale = a.keys / nk
    dev_s = float(np.median(t_call))
    host_s = (t_host_ms + t_host_seq) * scale
    rec = {
        "metric": "sequence score and fixation edit distance of a validation call (sequence_score_evaluation), seconds per call",
        "keys": a.keys, "human_scanpaths": len(gt), "predicted_scanpaths": len(pr), "fixations_per_scanpath": [3, 16],
        "points_per_key": [int(min(map(len, pooled))), int(max(map(len, pooled)))], "pairs": int(len(pairs)), "bandwidth": h, "gap": 0.0,
        "max_iter": 300, "clusters_per_key_mean": float(np.mean([len(c[0]) for c in clusters])),
        "kernel_shape": "mean shift: one 256-thread block per key, one thread per seed; strings: one lane per fixation; SS / FED: one "
                        "wavefront per pair (csrc/seqscore.hip)",
        "device_s": dev_s, "device_s_all": [float(t) for t in t_call],
        "device_meanshift_clusters_s": float(np.median(t_ms)), "device_cluster_strings_s": float(np.median(t_str)),
        "device_sequence_scores_pairs_s": float(np.median(t_seq)),
        "device_kind": "host clock around the whole call: packing, one upload, 3 launches, one copy back (synchronises), per-key grouping "
                       "on the host; the three batched calls alone each include their own packing, upload and copy back",
        "host_s": host_s, "host_keys_timed": int(nk), "host_meanshift_s_timed": t_host_ms, "host_strings_and_pairs_s_timed": t_host_seq,
        "host_pairs_timed": int(len(sel)),
        "host_kind": "tests/seqscore_ref.py (plain Python loops over floats, one core) over a seeded random subset of the keys, scaled to "
                     "all keys",
        "host_over_device": host_s / dev_s,
        "host_sklearn_meanshift_s": None if t_sk is None else t_sk * scale, "host_sklearn_meanshift_s_timed": t_sk,
        "host_sklearn_kind": "sklearn.cluster.MeanShift(bin_seeding=False, cluster_all=True).fit once per key of the same subset, scaled; "
                             "clustering only (null: sklearn is not installed)",
        "host_sklearn_plus_loop_pairs_s": None if t_sk is None else (t_sk + t_host_seq) * scale,
        "host_sklearn_plus_loop_pairs_over_device": None if t_sk is None else (t_sk + t_host_seq) * scale / dev_s,
        "differing_host_vs_device": differ, "means": {k: v for k, v in means.items()},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
