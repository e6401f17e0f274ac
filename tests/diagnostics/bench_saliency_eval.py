"""Saliency scoring of a validation call: scanpath_saliency on the device against the same work on the host -- numpy rasterisation,
scipy.ndimage.gaussian_filter and the per-map wrappers AUC_Judd / NSS / KLdiv (one upload and one launch per map and metric, what a
caller had before evaltools/saliency_maps.py).  Workload: 500 questions at 240x320, sigma 10, 3-10 human and 20 predicted scanpaths
per question.
    python tests/diagnostics/bench_saliency_eval.py [--questions 500] [--host-questions 500] [--reps 5] [--out profiles/bench_saliency_eval.json]
The device time is a host clock around calls that end in a device synchronise (fixation upload and host-side packing included);
every shape is warmed up first.  Entry-point calls are counted through the binding; launches = calls x launches per entry point.
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

LAUNCHES = {"sp_fixation_maps": 1, "sp_gaussian_blur_maps": 2, "sp_count_positive": 1, "sp_saliency_metrics": 1}


def workload(questions, g):
    def scanpath():
        n = int(g.integers(3, 13))
        return np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.08, 0.6, n)], 1)

    gt, gt_g, pr, pr_g = [], [], [], []
    for q in range(questions):
        nh = int(g.integers(3, 11))
        gt += [scanpath() for _ in range(nh)]
        gt_g += [q] * nh
        pr += [scanpath() for _ in range(20)]
        pr_g += [q] * 20
    return gt, gt_g, pr, pr_g


def host_maps(paths, groups, G, H, W):
    count = np.zeros((G, H, W))
    for p, q in zip(paths, groups):
        col = np.minimum(np.floor(p[:, 0] * W / 320.0).astype(np.int64), W - 1)
        row = np.minimum(np.floor(p[:, 1] * H / 240.0).astype(np.int64), H - 1)
        np.add.at(count[q], (row, col), 1.0)
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=500)
    ap.add_argument("--host-questions", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_saliency_eval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_saliency_eval needs a HIP device: a time taken elsewhere says nothing")
    from scipy.ndimage import gaussian_filter
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    H, W, G = 240, 320, a.questions
    gt, gt_g, pr, pr_g = workload(G, np.random.Generator(np.random.PCG64(0)))

    def device():
        res = M.scanpath_saliency(gt, gt_g, pr, pr_g, (H, W), a.sigma)
        out = {k: v.cpu().numpy() for k, v in res.items()}         # ends in a synchronise
        return out

    device()                                                        # warm-up: code objects, allocator, the LDS attribute
    calls = {}
    L = hip.lib()
    originals = {n: getattr(L, n) for n in LAUNCHES}
    for n, fn in originals.items():
        def counted(*args, _n=n, _fn=fn):
            calls[_n] = calls.get(_n, 0) + 1
            return _fn(*args)
        setattr(L, n, counted)
    dev_res = device()
    for n, fn in originals.items():
        setattr(L, n, fn)
    launches = sum(LAUNCHES[n] * c for n, c in calls.items())
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device()
        times.append(time.perf_counter() - t0)

    # the same work on the host, per map
    Gh = min(G, a.host_questions)
    keep_g = [k for k, q in enumerate(gt_g) if q < Gh]
    keep_p = [k for k, q in enumerate(pr_g) if q < Gh]
    t0 = time.perf_counter()
    hc = host_maps([gt[k] for k in keep_g], [gt_g[k] for k in keep_g], Gh, H, W)
    pc = host_maps([pr[k] for k in keep_p], [pr_g[k] for k in keep_p], Gh, H, W)
    host = {"AUC_Judd": np.zeros(Gh), "NSS": np.zeros(Gh), "KLdiv": np.zeros(Gh)}
    t_blur = 0.0
    for q in range(Gh):
        t1 = time.perf_counter()
        pred = gaussian_filter(pc[q], a.sigma, mode="constant", cval=0.0, truncate=4.0)
        human = gaussian_filter(hc[q], a.sigma, mode="constant", cval=0.0, truncate=4.0)
        t_blur += time.perf_counter() - t1
        binary = (hc[q] > 0).astype(np.float64)
        host["AUC_Judd"][q] = M.AUC_Judd(pred, binary, jitter=False)
        host["NSS"][q] = M.NSS(pred, binary)
        host["KLdiv"][q] = M.KLdiv(pred, human)
    t_host = time.perf_counter() - t0
    diff = {k: float(np.nanmax(np.abs(host[k] - dev_res[k][:Gh]))) for k in host}
    dev_s = float(np.median(times))
    host_s = t_host * G / Gh
    rec = {
        "metric": "saliency scoring of a validation call (AUC_Judd, NSS, KLdiv per question), seconds per call",
        "questions": G, "map": [H, W], "sigma": a.sigma, "human_scanpaths": len(gt), "predicted_scanpaths": len(pr),
        "device_s": dev_s, "device_s_all": [float(t) for t in times], "device_entry_point_calls": calls, "device_launches": launches,
        "host_s": host_s, "host_questions_timed": Gh, "host_blur_s": t_blur * G / Gh,
        "host_kind": "numpy np.add.at + scipy gaussian_filter + per-map AUC_Judd / NSS / KLdiv wrappers (3 launches and 6 map uploads per question)",
        "host_over_device": host_s / dev_s, "max_abs_difference_host_vs_device": diff,
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
