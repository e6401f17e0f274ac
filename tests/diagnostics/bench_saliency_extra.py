"""Cost of the shuffled AUC / CC / SIM / information gain next to the saliency scoring of a validation call, on the workload of
bench_saliency_eval.py (500 questions at 240x320, sigma 10, 3-10 human and 20 predicted scanpaths per question; four questions per
image here).
    python tests/diagnostics/bench_saliency_extra.py [--questions 500] [--reps 5] [--rounds 5] [--parent-root DIR]
                                                     [--out profiles/bench_saliency_extra.json]
Records seconds per call of scanpath_saliency without extras, with all four extras, of the human-ceiling call
(evaluation.saliency_human_evaluation) and of the centre-prior call, the entry-point calls and launches of each, and the host time of
the numpy checker (tests/saliency_ext_ref.py) for the four extras on the very maps the device scored.
--parent-root DIR: a built checkout of the parent commit.  The call WITHOUT extras is then timed in fresh child processes, parent and
this tree in turn for --rounds rounds (that path is meant to be untouched: this tree's median has to lie inside the parent's min-max
spread); both series go into the file.
Times are a host clock around calls that end in a device synchronise; every shape is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LAUNCHES = {"sp_fixation_maps": 1, "sp_gaussian_blur_maps": 2, "sp_count_positive": 1, "sp_saliency_metrics": 1,
            "sp_fixation_pool_counts": 1, "sp_saliency_scores": 1}
ALL = ("sAUC", "CC", "SIM", "IG")


def plain_worker(root, questions, reps, sigma):
    """(child process) seconds per scanpath_saliency call without extras, on the package under `root`"""
    sys.path.insert(0, root)
    sys.path.insert(1, HERE)
    import torch
    from bench_saliency_eval import workload
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    gt, gt_g, pr, pr_g = workload(questions, np.random.Generator(np.random.PCG64(0)))

    def call():
        return {k: v.cpu().numpy() for k, v in M.scanpath_saliency(gt, gt_g, pr, pr_g, (240, 320), sigma).items()}

    call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    print(json.dumps({"root": root, "times": times}))


def timed(fn, reps):
    import torch
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return times


def counted(fn):
    from scanpaths_amd import hip
    L = hip.lib()
    calls = {}
    originals = {n: getattr(L, n) for n in LAUNCHES}
    for n, f in originals.items():
        def wrapper(*args, _n=n, _f=f):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*args)
        setattr(L, n, wrapper)
    try:
        fn()
    finally:
        for n, f in originals.items():
            setattr(L, n, f)
    return {"entry_point_calls": calls, "launches": sum(LAUNCHES[n] * c for n, c in calls.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--uniform-mix", type=float, default=0.01)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--worker-root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_saliency_extra.json"))
    a = ap.parse_args()
    if a.worker_root:
        return plain_worker(a.worker_root, a.questions, a.reps, a.sigma)
    sys.path.insert(0, ROOT)
    sys.path.insert(1, HERE)
    sys.path.insert(2, os.path.dirname(HERE))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_saliency_extra needs a HIP device: a time taken elsewhere says nothing")
    import saliency_ext_ref as R
    from bench_saliency_eval import workload
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import saliency_maps as SM
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    H, W, G = 240, 320, a.questions
    gt, gt_g, pr, pr_g = workload(G, np.random.Generator(np.random.PCG64(0)))
    images = [q // 4 for q in range(G)]
    extra = dict(extra_metrics=ALL, image_groups=images, uniform_mix=a.uniform_mix)

    def sync(res):
        return {k: v.cpu().numpy() for k, v in res.items()}

    plain = lambda: sync(M.scanpath_saliency(gt, gt_g, pr, pr_g, (H, W), a.sigma))
    full = lambda: sync(M.scanpath_saliency(gt, gt_g, pr, pr_g, (H, W), a.sigma, **extra))
    floor = lambda: sync(M.scanpath_saliency(gt, gt_g, [], [], (H, W), a.sigma, prediction="centre_prior", **extra))
    human = lambda: E.saliency_human_evaluation(gt, gt_g, (H, W), sigma=a.sigma, extra_metrics=ALL, image_keys=[images[q] for q in gt_g],
                                                uniform_mix=a.uniform_mix)
    rec = {"metric": "saliency scoring of a validation call with sAUC, CC, SIM and IG, seconds per call (median)",
           "questions": G, "images": len(set(images)), "map": [H, W], "sigma": a.sigma, "uniform_mix": a.uniform_mix,
           "human_scanpaths": len(gt), "predicted_scanpaths": len(pr)}
    for name, fn in (("without_extras", plain), ("with_all_extras", full), ("centre_prior", floor), ("human_ceiling", human)):
        t = timed(fn, a.reps)
        rec[name] = {"s": float(np.median(t)), "s_all": [float(v) for v in t], **counted(fn)}
    rec["extras_cost_s"] = rec["with_all_extras"]["s"] - rec["without_extras"]["s"]

    # the checker on the maps the device scored: the four extras per question, in numpy on one core
    dev = torch.device("cuda", torch.cuda.current_device())
    up = SM._Upload(list(gt) + list(pr), np.concatenate([np.asarray(gt_g), np.asarray(pr_g) + G]), 2 * G, dev)
    counts, _ = up.rasterise((H, W), None, "count")
    dens = SM.density_maps(counts, a.sigma).cpu().numpy()
    c = counts[:G].cpu().numpy()
    b = (c > 0).astype(np.float64)
    Ei = max(images) + 1
    per_image = np.zeros((Ei, H, W))
    np.add.at(per_image, np.asarray(images), c)
    base = SM.density_maps(per_image.sum(0)[None] - per_image, a.sigma).cpu().numpy()
    t0 = time.perf_counter()
    cnt, tot = R.pool_counts(b, images, Ei)
    host = {m: np.zeros(G) for m in ALL}
    with np.errstate(all="ignore"):
        for q in range(G):
            S, D, B = dens[G + q], dens[q], base[images[q]]
            host["sAUC"][q] = R.sauc(S, b[q], tot - cnt[images[q]])
            host["CC"][q], host["SIM"][q], host["IG"][q] = R.cc(S, D), R.sim(S, D), R.infogain(S, b[q], B, a.uniform_mix)
    rec["checker_host_s"] = time.perf_counter() - t0
    rec["checker_kind"] = "numpy restatement (tests/saliency_ext_ref.py) of the four extras on the device's maps, one core; no rasterisation, no blur"
    got = full()
    with np.errstate(all="ignore"):
        rec["max_abs_difference_checker_vs_device"] = {m: float(np.nanmax(np.abs(host[m] - got[m]))) for m in ALL}
    rec["nan_patterns_equal"] = bool(all(np.array_equal(np.isnan(host[m]), np.isnan(got[m])) for m in ALL))

    if a.parent_root:
        series = {"parent": [], "this": []}
        for _ in range(a.rounds):
            for tag, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker-root", root, "--questions", str(G), "--reps",
                                      str(a.reps), "--sigma", str(a.sigma)], check=True, capture_output=True, text=True, timeout=300)
                series[tag].append(float(np.median(json.loads(out.stdout.strip().splitlines()[-1])["times"])))
        med = float(np.median(series["this"]))
        rec["without_extras_vs_parent"] = {
            "what": "scanpath_saliency without extras, median seconds per call of a fresh process; parent commit and this tree in turn",
            "parent_s": series["parent"], "this_s": series["this"], "this_median_s": med,
            "parent_min_s": min(series["parent"]), "parent_max_s": max(series["parent"]),
            "this_median_inside_parent_spread": bool(min(series["parent"]) <= med <= max(series["parent"]))}
    rec["box"] = f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}"
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
