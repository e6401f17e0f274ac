"""MultiMatch with scanpath simplification (grouping) in a validation call: evaluation_performance_related with
multimatch_grouping on the device default (sp_scan_simplify + sp_scan_multimatch_gated, every pair of the call in two launches) against
the same call with the host callable (utils/evaltools/multimatch.docomparison, grouping=True, one pair at a time on one core), and
simplify_scanpaths alone against the host loop over simplify_scanpath.  Workload: --images images, 3-10 human scanpaths and one
prediction each, 3-16 fixations in a 320x240 frame, half of the scanpaths on an 8 px lattice; thresholds (45 degrees, 0.3, 40 px).
    python tests/diagnostics/bench_multimatch_simplify.py [--images 500] [--host-images 50] [--reps 5] [--out profiles/bench_multimatch_simplify.json]
The device times are host clocks around whole calls (packing, upload, launches, the copy back, which synchronises; for the keyed call
also ScanMatch, SED / STDE and the grouping on the host, which both sides share).  One warm-up call comes first.  The host time of the
keyed call is taken over the first --host-images images and scaled to all of them (0: all).  Prints one JSON line and writes it to --out."""
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

FV = {"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")}
THRESHOLDS = (45.0, 0.3, 40.0)


def workload(images, g):
    def scanpath(lattice):
        n = int(g.integers(3, 17))
        a = np.zeros(n, dtype=FV)
        if lattice:
            a["start_x"], a["start_y"], a["duration"] = g.integers(0, 40, n) * 8.0, g.integers(0, 30, n) * 8.0, g.integers(1, 7, n) * 0.1
        else:
            a["start_x"], a["start_y"], a["duration"] = g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.05, 0.6, n)
        return a

    gt = [[scanpath(bool((q + j) % 2)) for j in range(int(g.integers(3, 11)))] for q in range(images)]
    pred = [scanpath(bool(q % 2)) for q in range(images)]
    perf = [[bool(g.random() < 0.5) for _ in x] for x in gt]
    perf[0], perf[1] = [True] * len(perf[0]), [False] * len(perf[1])
    alloc = [bool(q % 2 == 0) for q in range(images)]
    return gt, pred, perf, alloc


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
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--host-images", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_multimatch_simplify.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multimatch_simplify needs a HIP device: a time taken elsewhere says nothing")
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import multimatch as M
    gt, pred, perf, alloc = workload(a.images, np.random.Generator(np.random.PCG64(0)))
    tdir, tdur, tamp = THRESHOLDS
    paths, pairs = [], []
    for q in range(a.images):
        for h in gt[q]:
            paths += [h, pred[q]]
            pairs.append((len(paths) - 2, len(paths) - 1))

    def keyed(n, **kw):
        return E.evaluation_performance_related(gt[:n], pred[:n], perf[:n], alloc[:n], multimatch_grouping=THRESHOLDS, **kw)

    keyed(a.images)                                                   # warm-up: code objects, allocator
    dev_out, t_call = timed(lambda: keyed(a.images), a.reps)
    _, t_plain = timed(lambda: E.evaluation_performance_related(gt, pred, perf, alloc), a.reps)
    dev_mm, t_mm = timed(lambda: M.multimatch_pairs(paths, pairs, [320, 240], grouping=True, TDir=tdir, TDur=tdur, TAmp=tamp), a.reps)
    dev_simple, t_simple = timed(lambda: M.simplify_scanpaths(paths, TDir=tdir, TDur=tdur, TAmp=tamp), a.reps)

    nh = a.images if a.host_images <= 0 else min(a.host_images, a.images)
    with np.errstate(all="ignore"):
        t0 = time.perf_counter()
        keyed(nh, multimatch=M.docomparison)
        t_host_call = time.perf_counter() - t0
        npair_h = sum(len(x) for x in gt[:nh])
        t0 = time.perf_counter()
        host_mm = np.array([M.docomparison(paths[i], paths[j], [320, 240], True, tdir, tdur, tamp) for i, j in pairs[:npair_h]])
        t_host_mm = time.perf_counter() - t0
    _, t_sub = timed(lambda: keyed(nh), a.reps)
    t0 = time.perf_counter()
    host_simple = [M.simplify_scanpath(p, tdir, tdur, tamp) for p in paths]
    t_host_simple = time.perf_counter() - t0
    differ = int(sum(not np.array_equal(x, y) for x, y in zip(host_simple, dev_simple)))
    scale = a.images / nh
    dev_s = float(np.median(t_call))
    rec = {
        "metric": "evaluation_performance_related with multimatch_grouping=(45, 0.3, 40), seconds per call",
        "images": a.images, "human_scanpaths": int(sum(len(x) for x in gt)), "pairs": len(pairs), "fixations_per_scanpath": [3, 16],
        "thresholds": list(THRESHOLDS), "scanpaths_simplified": len(paths),
        "fixations_before": int(sum(len(p) for p in paths)), "fixations_after": int(sum(len(p) for p in dev_simple)),
        "kernel_shape": "simplification: one wavefront per scanpath, one lane per fixation, four per 256-thread block "
                        "(csrc/scansimplify.hip); MultiMatch: one thread per pair (csrc/scanmetrics.hip)",
        "device_s": dev_s, "device_s_all": [float(t) for t in t_call],
        "device_ungrouped_call_s": float(np.median(t_plain)),
        "device_multimatch_pairs_grouped_s": float(np.median(t_mm)), "device_simplify_scanpaths_s": float(np.median(t_simple)),
        "device_kind": "host clock around the whole call: packing, upload, launches, copy back (synchronises); the keyed call also runs "
                       "ScanMatch, SED / STDE and the per-image grouping on the host, which the host side shares",
        "host_s": t_host_call * scale, "host_images_timed": int(nh), "host_s_timed": t_host_call,
        "device_s_same_images": float(np.median(t_sub)),
        "host_multimatch_pairs_s": t_host_mm * scale, "host_multimatch_pairs_timed": int(npair_h),
        "host_simplify_s": t_host_simple,
        "host_kind": "the same keyed call with multimatch=docomparison (numpy and Python loops, one pair at a time, one core) over the "
                     "first images, scaled to all; simplify_scanpath over every scanpath",
        "host_over_device": t_host_call * scale / dev_s,
        "host_over_device_multimatch_pairs": t_host_mm * scale / float(np.median(t_mm)),
        "host_over_device_simplify": t_host_simple / float(np.median(t_simple)),
        "simplified_scanpaths_differing_host_vs_device": differ,
        "worst_multimatch_diff_host_vs_device": [float(v) for v in np.nanmax(np.abs(host_mm - dev_mm[:npair_h]), 0)],
        "means": {k: float(v) for k, v in dev_out[0]["all"]["MultiMatch"].items()},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
