"""Recurrence statistics at the size of a validation pass: two routes to the SAME recurrence table for the same rows of step
distributions -- the closed form (evaltools/recurrence_statistics.recurrence_expectation: exact, no sampling noise) and the sampled
route (10 samples per row through Sampling.random_sample / generate_scanpath, then recurrence_counts).  Workload: 600 rows x 16 steps
x 1201 actions (the 30 x 40 map on 240 x 320), radius 16 px, min_length 1, max_steps 16, min_line 2.
    python tests/diagnostics/bench_recurrence_statistics.py [--rows 600] [--samples 10] [--reps 20] [--sampled-reps 5]
                                                            [--out profiles/bench_recurrence_statistics.json]
Both times are a host clock around the whole route, ending in the copy back that synchronises; the distributions are on the device
before the clock starts, as they are after a forward.  The closed form: the upload of the row groups and the mask, the four launches,
one copy back of the table.  The sampled route: per sample one sp_sample_actions and two sp_generate_scanpath launches with their
copies and the host loop that builds the fixation vectors (what run_test_loop does), then ONE recurrence_counts call for all samples.
One warm-up of each route comes first; the median and the min-max of the timed calls are reported next to every single time.  L1_by_lag
and JSD_lag between the two tables are sanity figures: they are the sampling noise of rows x samples scanpaths, not an error.  No speed
bar is set: the closed form's case is exactness, the sampled route is the yardstick that gets reported.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sampled-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_recurrence_statistics.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recurrence_statistics needs a HIP device: a time taken elsewhere says nothing")
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.utils.evaltools import recurrence_statistics as M
    T, shape, frame, min_length, max_steps, radius, min_line = 16, (30, 40), (240, 320), 1, 16, 16.0, 2
    P = shape[0] * shape[1]
    g = np.random.Generator(np.random.PCG64(0))
    dev = torch.device("cuda", torch.cuda.current_device())
    d_probs = torch.softmax(torch.from_numpy(g.normal(0, 3, (a.rows, T, 1 + P)).astype(np.float32)).to(dev), 2)
    d_mu = torch.zeros(a.rows, T, device=dev)
    d_s2 = torch.full((a.rows, T), 0.1, device=dev)
    images = torch.zeros(1)
    sampler = Sampling(convLSTM_length=T, min_length=min_length, map_width=shape[1], map_height=shape[0], width=frame[1], height=frame[0],
                       seed=0)
    groups = np.zeros(a.rows, dtype=np.int64)
    ones = int(M.recurrence_mask(shape, frame, radius).sum())

    def closed():
        return M.recurrence_expectation(d_probs, groups, 1, min_length=min_length, max_steps=max_steps, radius=radius, frame_size=frame,
                                        map_shape=shape)

    def sampled():
        fvs = []
        for _ in range(a.samples):
            s = sampler.random_sample(d_probs, d_mu, d_s2)
            fvs += sampler.generate_scanpath(images, s["selected_actions_probs"], s["durations"], s["selected_actions"])[0]
        return M.recurrence_counts(fvs, np.zeros(len(fvs), dtype=np.int64), 1, frame, shape, max_steps=max_steps, radius=radius,
                                   min_line=min_line)

    exact, counted = closed(), sampled()                   # warm-up: code objects, allocator
    t_closed, t_sampled = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exact = closed()
        t_closed.append(time.perf_counter() - t0)
    for _ in range(a.sampled_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counted = sampled()
        t_sampled.append(time.perf_counter() - t0)
    s_exact, s_counted = M.recurrence_summary(exact["E"][0]), M.recurrence_summary(counted["counts"][0])
    cmp_ = M.recurrence_comparison(exact["E"][0], counted["counts"][0])
    measures = M.recurrence_measures(counted["rqa"])
    pairs = T * (T - 1) // 2
    rec = {
        "metric": "recurrence statistics of one validation-sized pass: two routes to one recurrence table, seconds per route",
        "rows": a.rows, "steps": T, "actions": 1 + P, "map_shape": list(shape), "frame_size": list(frame), "radius_px": radius,
        "mask_ones": ones, "min_length": min_length, "max_steps": max_steps, "min_line": min_line, "samples_per_row": a.samples,
        "sampled_scanpaths": int(len(counted["points"])),
        "kernel_shape": "recurrence_expectation: one launch that lists the mask's displacements, one 256-thread block per (row, step) with "
                        "the step's map and its blurred map in LDS as doubles, the waves sharing out the earlier steps, then one thread "
                        "per row and per (group, entry); recurrence_counts: one wavefront per scanpath, one ballot per row of the plot, "
                        "integer atomics (csrc/scanrecur.hip)",
        "recurrence_expectation_s": float(np.median(t_closed)), "recurrence_expectation_s_all": [float(t) for t in t_closed],
        "recurrence_expectation_s_min_max": [float(min(t_closed)), float(max(t_closed))], "recurrence_expectation_timed_calls": len(t_closed),
        "sampled_route_s": float(np.median(t_sampled)), "sampled_route_s_all": [float(t) for t in t_sampled],
        "sampled_route_s_min_max": [float(min(t_sampled)), float(max(t_sampled))], "sampled_route_timed_calls": len(t_sampled),
        "closed_form_is_faster": bool(np.median(t_closed) < np.median(t_sampled)),
        "device_kind": "host clock around each whole route, ending in the copy back that synchronises; one warm-up each",
        "closed_form_blur_additions": int(a.rows * T * P * ones), "closed_form_map_products": int(a.rows * pairs * P),
        "device_scratch_bytes": int((a.rows * T * T + (2 * shape[0] - 1) * (2 * shape[1] - 1) // 2 + 1) * 8),
        "bytes_copied_back_closed_form": int(max_steps * max_steps * 8 + 12 * a.rows),
        "rows_bad": int((exact["bad"] != 0).sum()), "expected_points": float(exact["points"].sum()),
        "sampled_points_per_sample_of_all_rows": float(counted["points"].sum() / a.samples),
        "L1_by_lag_closed_vs_sampled": cmp_["L1_by_lag"], "JSD_lag_closed_vs_sampled_bits": cmp_["JSD_lag"],
        "REC_difference_closed_minus_sampled": cmp_["REC_difference"],
        "REC": {"closed_form": s_exact["REC"], "sampled": s_counted["REC"]},
        "mean_lag": {"closed_form": s_exact["mean_lag"], "sampled": s_counted["mean_lag"], "chance_closed_form": s_exact["mean_lag_chance"]},
        "recurrence_by_lag": {"closed_form": s_exact["recurrence_by_lag"].tolist(), "sampled": s_counted["recurrence_by_lag"].tolist()},
        "sampled_only_line_measures_mean": {k: float(np.nanmean(measures[k])) if not np.isnan(measures[k]).all() else None
                                            for k in ("DET", "LAM")},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
