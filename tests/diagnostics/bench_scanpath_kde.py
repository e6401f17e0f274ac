"""The KDE centre-bias baseline and the human gold standard at validation-set size: evaltools.scanpath_kde on the device against the host
path -- the vectorised `quick` numpy restatement of tests/scanpath_kde_ref.py, the fastest host form that its plain-loop twin holds to
the same values.  Workload: 1,500 images x 15 scanpaths of 3-16 fixations around three hot spots per image in a 320x240 frame, the
30 x 40 map, 16 bandwidths from 4 to 128 px, uniform_mix 0.01: one kde_bandwidth_search per leave mode and one kde_cell_baselines.
    python tests/diagnostics/bench_scanpath_kde.py [--images 1500] [--subjects 15] [--reps 5] [--host-images N] [--out profiles/bench_scanpath_kde.json]
The device time is a host clock around each whole call: packing, the one upload, the launches, the one copy back (which synchronises) and
the pooling on the host (kde_cell_baselines returns a device tensor: the clock stops after a synchronize).  One warm-up call comes first,
then --reps calls: median and min-max.  The host form takes tens of seconds at this size, so it is timed ONCE, on the first --host-images
images (default: all of them); the device is timed on the same images next to it, and the differences between the two paths are taken
there (a leave="image" score depends on which other images are in the call, so the two must see the same ones).  The kernels' own
times are not measured.  Prints one JSON line and writes it to --out."""
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


def workload(images, subjects, g, frame=(240.0, 320.0)):
    h, w = frame
    paths, groups = [], []
    for i in range(images):
        spots = g.uniform(0.15, 0.85, (3, 2)) * (w, h)
        for _ in range(subjects):
            n = int(g.integers(3, 17))
            xy = np.clip(spots[g.integers(0, 3, n)] + g.normal(0, 0.07, (n, 2)) * (w, h), 0.0, (w - 0.5, h - 0.5))
            paths.append(np.concatenate([xy, g.uniform(0.08, 0.6, (n, 1))], 1))
            groups.append(i)
    return paths, groups


def clock(fn, reps):
    out = None
    fn()                                                 # warm-up: code object, allocator
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, dict(median_s=float(np.median(times)), min_s=float(min(times)), max_s=float(max(times)), all_s=[float(t) for t in times])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1500)
    ap.add_argument("--subjects", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_scanpath_kde.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scanpath_kde needs a HIP device: a time taken elsewhere says nothing")
    import scanpath_kde_ref as R
    from scanpaths_amd.utils.evaltools import scanpath_kde as M
    shape, frame, u = (30, 40), (240.0, 320.0), 0.01
    bws = np.geomspace(4.0, 128.0, 16)
    paths, groups = workload(a.images, a.subjects, np.random.Generator(np.random.PCG64(0)))
    a.host_images = a.host_images if 0 < a.host_images < a.images else a.images
    few = sum(1 for g in groups if g < a.host_images)
    sizes = {"full": (paths, groups)}
    if few < len(paths):
        sizes["fraction"] = (paths[:few], groups[:few])
    hsize = "fraction" if few < len(paths) else "full"
    calls = {leave: (lambda p, g, leave=leave: M.kde_bandwidth_search(p, g, frame, shape, bandwidths=bws, uniform_mix=u, leave=leave))
             for leave in M.LEAVE}
    calls["baselines"] = lambda p, g: M.kde_cell_baselines(p, g, frame, shape, bandwidth=float(bws[8]))
    device, results = {}, {}
    for size, (p, g) in sizes.items():
        for name, call in calls.items():
            results[size, name], device[f"{name}_{size}"] = clock(lambda: call(p, g), a.reps)
    host, worst = {}, {}
    p, g = sizes[hsize]
    for name in calls:
        t0 = time.perf_counter()
        ref = R.quick_baselines(p, g, frame, shape, float(bws[8])) if name == "baselines" else R.search(p, g, frame, shape, bws, u, name)
        host[name] = time.perf_counter() - t0
        got = results[hsize, name]
        if name == "baselines":
            total = ref.sum(0) / max(a.host_images - 1, 1)                            # every fixation is in all rows but its own image's
            worst[name] = {"cells_over_cell_total": float((np.abs(got.cpu().numpy() - ref) / np.maximum(total, 1e-300)).max())}
        else:
            worst[name] = {"mean_bits": float((np.abs(got["LL"] - ref["LL"]) / np.maximum(1.0, np.abs(ref["LL"]))).max()),
                           "same_best": bool(got["best"] == ref["best"]), "same_count": bool(got["count"] == ref["count"])}
    full = {name: results["full", name] for name in M.LEAVE}
    rec = {
        "metric": "KDE centre-bias baseline and gold standard at validation-set size, seconds per call",
        "images": a.images, "subjects_per_image": a.subjects, "scanpaths": len(paths), "fixations": int(sum(len(p) for p in paths)),
        "map": list(shape), "bandwidths": [float(b) for b in bws], "uniform_mix": u, "baseline_bandwidth": float(bws[8]),
        "kernel_shape": "prologue: one thread per (fixation, bandwidth); tables: one block per (image, bandwidth), prefix + suffix over the "
                        "images; pairs: one thread per (fixation, bandwidth), sources of the image through LDS in tiles of 32 (csrc/scankde.hip)",
        "device": device,
        "device_kind": "host clock around the whole call: packing, one upload, the launches, one copy back (synchronises), pooling on the "
                       "host; one warm-up, then the median / min / max of the repetitions",
        "search_full": {k: {"best": v["best"], "count": v["count"], "mean_bits": [float(x) for x in v["LL"]]} for k, v in full.items()},
        "host_images": a.host_images, "host_fixations": int(sum(len(p) for p in sizes[hsize][0])), "host_s_once": host,
        "host_kind": "tests/scanpath_kde_ref.py quick form (numpy, one process), timed ONCE on the first host_images images",
        "host_over_device": {k: host[k] / device[f"{k}_{hsize}"]["median_s"] for k in host},
        "worst_difference_host_vs_device": worst,
        "not_measured": "the kernels' own times; repetitions of the host form",
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}",
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
