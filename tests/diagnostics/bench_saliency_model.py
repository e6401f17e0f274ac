"""Saliency scores of the model at the size of a validation pass: two routes to the SAME scores (AUC_Judd, NSS, KLdiv, CC, SIM) for the
same rows of step distributions -- the closed form (evaltools/saliency_maps.expected_fixation_maps -> scanpath_saliency with
prediction="maps", through utils.evaluation.saliency_model_evaluation: exact, no sampling noise) and the sampled route (10 samples per
row through Sampling.random_sample / generate_scanpath, then utils.evaluation.saliency_evaluation).  Workload: 600 rows x 16 steps x 1201
actions (the 30 x 40 map on 240 x 320), one key per row, three synthetic human scanpaths per key (so the keyed closed form reads every
row three times, once per subject), sigma 8 px, min_length 1, max_steps 16.
    python tests/diagnostics/bench_saliency_model.py [--rows 600] [--samples 10] [--reps 10] [--sampled-reps 3]
                                                     [--out profiles/bench_saliency_model.json]
All times are a host clock around the whole route, ending in the copy back that synchronises; the distributions are on the device
before the clock starts, as they are after a forward.  expected_fixation_maps alone: the upload of the row groups and the cell-pixel
table, the four launches, the copy back of fixations and bad (the maps stay on the device).  Closed form to the scores: that, the
upload of the human scanpaths, the rasterisation, blur and metric launches and the copy back of the scores.  The sampled route: per
sample one sp_sample_actions and two sp_generate_scanpath launches with their copies and the host loop that builds the fixation vectors
(what run_test_loop does), then ONE saliency_evaluation call.  One warm-up of each route comes first (it also makes the cell-pixel
table); the median and the min-max of the timed calls are reported next to every single time.  The per-metric mean absolute difference
between the two routes' per-key scores is the sampling noise of `samples` scanpaths per key, not an error.  No speed bar is set: the
closed form's case is exactness, the sampled route is the yardstick that gets reported.
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
METRICS = ("AUC_Judd", "NSS", "KLdiv", "CC", "SIM")


def timed(fn, reps):
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def report(name, times):
    return {name + "_s": float(np.median(times)), name + "_s_all": [float(t) for t in times],
            name + "_s_min_max": [float(min(times)), float(max(times))], name + "_timed_calls": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sampled-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_saliency_model.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_saliency_model needs a HIP device: a time taken elsewhere says nothing")
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import saliency_maps as S
    T, shape, frame, min_length, max_steps, sigma, subjects = 16, (30, 40), (240, 320), 1, 16, 8.0, 3
    P = shape[0] * shape[1]
    g = np.random.Generator(np.random.PCG64(0))
    dev = torch.device("cuda", torch.cuda.current_device())
    predict = {"all_actions_prob": torch.softmax(torch.from_numpy(g.normal(0, 3, (a.rows, T, 1 + P)).astype(np.float32)).to(dev), 2),
               "log_normal_mu": torch.zeros(a.rows, T, device=dev), "log_normal_sigma2": torch.full((a.rows, T), 0.1, device=dev)}
    keys = [f"q{i}" for i in range(a.rows)]
    humans = [[np.stack([g.uniform(0, frame[1], n), g.uniform(0, frame[0], n), g.uniform(0.1, 0.5, n)], 1) for n in g.integers(3, 12, subjects)]
              for _ in keys]
    flat, flat_keys = [fv for s in humans for fv in s], [k for k, s in zip(keys, humans) for _ in s]
    images = torch.zeros(1)
    sampler = Sampling(convLSTM_length=T, min_length=min_length, map_width=shape[1], map_height=shape[0], width=frame[1], height=frame[0],
                       seed=0)
    groups = np.arange(a.rows, dtype=np.int64)

    def maps_alone():
        return S.expected_fixation_maps(predict["all_actions_prob"], groups, a.rows, min_length=min_length, max_steps=max_steps,
                                        frame_size=frame)

    def closed():
        # one model row per subject (a head read by k subjects counts k times): rows x subjects rows go through the expectation
        return E.saliency_model_evaluation(predict, humans, keys, sigma=sigma, min_length=min_length, max_steps=max_steps,
                                           frame_size=frame, extra_metrics=("CC", "SIM"))

    def sampled():
        fvs, pk = [], []
        for _ in range(a.samples):
            s = sampler.random_sample(predict["all_actions_prob"], predict["log_normal_mu"], predict["log_normal_sigma2"])
            fvs += sampler.generate_scanpath(images, s["selected_actions_probs"], s["durations"], s["selected_actions"])[0]
            pk += keys
        return E.saliency_evaluation(flat, fvs, flat_keys, pk, frame, sigma=sigma, extra_metrics=("CC", "SIM"))

    maps_alone(), closed(), sampled()                       # warm-up: code objects, allocator, the cell-pixel table
    res, t_maps = timed(maps_alone, a.reps)
    (c_means, c_keys), t_closed = timed(closed, a.reps)
    (s_means, s_keys), t_sampled = timed(sampled, a.sampled_reps)
    assert c_keys["keys"] == s_keys["keys"] == keys
    with np.errstate(invalid="ignore"):
        noise = {m: float(np.nanmean(np.abs(c_keys[m] - s_keys[m]))) for m in METRICS}
    rec = {
        "metric": "saliency scores of the model over one validation-sized pass: two routes to the same scores, seconds per route",
        "rows": a.rows, "steps": T, "actions": 1 + P, "map_shape": list(shape), "frame_size": list(frame), "keys": a.rows,
        "human_scanpaths": len(flat), "sigma_px": sigma, "min_length": min_length, "max_steps": max_steps, "samples_per_row": a.samples,
        "model_rows_closed_form": int(c_means["rows_count"] + c_means["rows_bad"]),
        "kernel_shape": "expected_fixation_maps: one wavefront per row for the step factors, one thread per cell for the (pixel, cell) "
                        "order, one thread per (group, cell) over the group's rows and steps, one thread per (group, pixel) over its "
                        "cells (csrc/scanexpect.hip); no LDS, no atomics",
        **report("expected_fixation_maps", t_maps), **report("closed_form_to_scores", t_closed), **report("sampled_route_to_scores", t_sampled),
        "closed_form_is_faster": bool(np.median(t_closed) < np.median(t_sampled)),
        "device_kind": "host clock around each whole route, synchronised at both ends; one warm-up each",
        "maps_bytes_on_device": int(a.rows * frame[0] * frame[1] * 8),
        "device_scratch_bytes_expectation": int((2 * a.rows * T + a.rows * P + P) * 8),
        "rows_bad": int((res["bad"] != 0).sum()), "expected_fixations_per_row": float(res["fixations"].mean()),
        "scores": {m: {"closed_form": float(c_means[m]), "sampled": float(s_means[m])} for m in METRICS},
        "mean_abs_difference_per_key_closed_vs_sampled": noise,
        "difference_is": f"the sampling noise of {a.samples} scanpaths per key, not an error",
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
