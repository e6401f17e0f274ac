"""DTW / Frechet / Hausdorff / Eyenalysis / REC / DET / LAM / CORM of a validation call: scanpath_distance_evaluation on the device
against the same pairs through the Python checker (tests/scanpath_dist_ref.py: plain double loops, what a caller had before
csrc/scandist.hip) on one core.  Workload: 500 keys, 3-10 human and 20 predicted scanpaths per key, 3-16 fixations each in a 320x240
frame -- the keys and scanpath counts of tests/diagnostics/bench_saliency_eval.py.
    python tests/diagnostics/bench_scanpath_distances.py [--keys 500] [--host-pairs 2000] [--reps 5] [--out profiles/bench_scanpath_distances.json]
The device time is a host clock around the whole call (fixation packing, the one upload, two launches, the one copy back, which
synchronises, and the per-key grouping on the host); the batched call alone (scanpath_distances_pairs) is timed as well.  One warm-up
call comes first.  The host time is the checker over a seeded random subset of --host-pairs pairs, scaled to all pairs (0: all of them).
Prints one JSON line and writes it to --out."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=500)
    ap.add_argument("--host-pairs", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=32.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_scanpath_distances.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scanpath_distances needs a HIP device: a time taken elsewhere says nothing")
    import scanpath_dist_ref as R
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    ALL = M.SCANPATH_DISTANCES
    gt, gt_k, pr, pr_k = workload(a.keys, np.random.Generator(np.random.PCG64(0)))
    # the pairs of the call, as scanpath_distance_evaluation forms them: (human scanpath of the key, prediction of the key)
    paths = [p[:, :2] for p in gt] + [p[:, :2] for p in pr]
    humans = {}
    for i, k in enumerate(gt_k):
        humans.setdefault(k, []).append(i)
    pairs = np.array([(i, len(gt) + j) for j, k in enumerate(pr_k) for i in humans[k]], dtype=np.int64)

    def call():
        return E.scanpath_distance_evaluation(gt, pr, gt_k, pr_k, metrics=ALL, radius=a.radius)

    def batch():
        return M.scanpath_distances_pairs(paths, pairs, metrics=ALL, radius=a.radius)

    call()                                                          # warm-up: code objects, allocator
    t_call, t_batch = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        means, _ = call()                                           # ends in the copy back
        t_call.append(time.perf_counter() - t0)
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = batch()
        t_batch.append(time.perf_counter() - t0)

    g = np.random.Generator(np.random.PCG64(1))
    nh = len(pairs) if a.host_pairs <= 0 else min(a.host_pairs, len(pairs))
    sub = np.sort(g.choice(len(pairs), nh, replace=False)) if nh < len(pairs) else np.arange(len(pairs))
    t0 = time.perf_counter()
    host = R.score_pairs(paths, pairs[sub], ALL, 1.0, a.radius, 2)
    t_host = time.perf_counter() - t0
    differ = {m: int((~((host[m] == dev[m][sub]) | (np.isnan(host[m]) & np.isnan(dev[m][sub])))).sum()) for m in ALL}
    dev_s, batch_s = float(np.median(t_call)), float(np.median(t_batch))
    host_s = t_host * len(pairs) / nh
    rec = {
        "metric": "DTW, Frechet, Hausdorff, Eyenalysis, REC, DET, LAM, CORM of a validation call (scanpath_distance_evaluation), seconds per call",
        "keys": a.keys, "human_scanpaths": len(gt), "predicted_scanpaths": len(pr), "fixations_per_scanpath": [3, 16], "pairs": int(len(pairs)),
        "radius": a.radius, "min_line": 2,
        "kernel_shape": "one wavefront per pair (csrc/scandist.hip); the one-thread-per-pair shape was not built and is unmeasured",
        "device_s": dev_s, "device_s_all": [float(t) for t in t_call],
        "device_batched_call_s": batch_s, "device_batched_call_s_all": [float(t) for t in t_batch],
        "device_kind": "host clock around the whole call: packing, one upload, 2 launches, one copy back (synchronises), per-key grouping on the host; "
                       "batched_call = scanpath_distances_pairs alone (no grouping)",
        "host_s": host_s, "host_pairs_timed": int(nh), "host_s_timed": t_host,
        "host_kind": "tests/scanpath_dist_ref.py (Python double loops over floats, one core) over a seeded random subset of the pairs, scaled to all pairs",
        "host_over_device": host_s / dev_s, "host_over_batched_call": host_s / batch_s,
        "pairs_differing_host_vs_device": differ, "means": {k: v for k, v in means.items()},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
