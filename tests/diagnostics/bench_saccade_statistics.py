"""Saccade statistics at the size of a validation pass: two routes to the SAME displacement lattice for the same rows of step
distributions -- the closed form (evaltools/saccade_statistics.saccade_expectation: exact, no sampling noise) and the sampled route (10
samples per row through Sampling.random_sample / generate_scanpath, then saccade_counts).  Workload: 600 rows x 16 steps x 1201 actions
(the 30 x 40 map on 240 x 320), min_length 1, max_steps 16.
    python tests/diagnostics/bench_saccade_statistics.py [--rows 600] [--samples 10] [--reps 7] [--out profiles/bench_saccade_statistics.json]
Both times are a host clock around the whole route, ending in the copy back that synchronises; the distributions are on the device
before the clock starts, as they are after a forward.  The closed form: the upload of the row groups, the two launches, one copy back of
the lattice.  The sampled route: per sample one sp_sample_actions and two sp_generate_scanpath launches with their copies and the host
loop that builds the fixation vectors (what run_test_loop does), then ONE saccade_counts call for all samples.  One warm-up of each
route comes first; the timed repeats alternate the two routes, and the medians are reported next to every single time.  The Jensen-
Shannon divergence between the two lattices is a sanity figure: it is the sampling noise of rows x samples scanpaths, not an error.
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_saccade_statistics.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_saccade_statistics needs a HIP device: a time taken elsewhere says nothing")
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.utils.evaltools import saccade_statistics as M
    T, shape, frame, min_length, max_steps = 16, (30, 40), (240, 320), 1, 16
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

    def closed():
        return M.saccade_expectation(d_probs, groups, 1, min_length=min_length, max_steps=max_steps, map_shape=shape)

    def sampled():
        fvs = []
        for _ in range(a.samples):
            s = sampler.random_sample(d_probs, d_mu, d_s2)
            fvs += sampler.generate_scanpath(images, s["selected_actions_probs"], s["durations"], s["selected_actions"])[0]
        return M.saccade_counts(fvs, np.zeros(len(fvs), dtype=np.int64), 1, frame, shape, max_steps=max_steps)

    exact, counted = closed(), sampled()                   # warm-up: code objects, allocator
    t_closed, t_sampled = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exact = closed()
        t_closed.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        counted = sampled()
        t_sampled.append(time.perf_counter() - t0)
    kw = dict(amplitude_edges=[0.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0], n_directions=8)
    s_exact, s_counted = M.saccade_summary(exact["E"][0], frame, **kw), M.saccade_summary(counted["counts"][0], frame, **kw)
    pairs = a.rows * (T - 1)
    rec = {
        "metric": "saccade statistics of one validation-sized pass: two routes to one displacement lattice, seconds per route",
        "rows": a.rows, "steps": T, "actions": 1 + P, "map_shape": list(shape), "min_length": min_length, "max_steps": max_steps,
        "samples_per_row": a.samples, "sampled_scanpaths": int(len(counted["saccades"])),
        "kernel_shape": "saccade_expectation: one 256-thread block per (row, 256 displacements), both step maps in LDS as doubles, one "
                        "thread per displacement, then one thread per (group, displacement) adds the rows; saccade_counts: one wavefront "
                        "per scanpath, integer atomics (csrc/scansaccade.hip)",
        "saccade_expectation_s": float(np.median(t_closed)), "saccade_expectation_s_all": [float(t) for t in t_closed],
        "sampled_route_s": float(np.median(t_sampled)), "sampled_route_s_all": [float(t) for t in t_sampled],
        "closed_form_is_faster": bool(np.median(t_closed) < np.median(t_sampled)),
        "device_kind": "host clock around each whole route, ending in the copy back that synchronises; routes alternate; one warm-up each",
        "closed_form_multiply_adds": int(pairs * P * P),
        "closed_form_multiply_adds_per_s_whole_call": float(pairs * P * P / np.median(t_closed)),
        "device_scratch_bytes": int(a.rows * 59 * 79 * 8), "bytes_copied_back_closed_form": int(59 * 79 * 8 + 12 * a.rows),
        "rows_bad": int((exact["bad"] != 0).sum()), "expected_saccades": float(exact["saccades"].sum()),
        "expected_saccades_lattice_total": float(exact["E"].sum()),
        "sampled_saccades_per_sample_of_all_rows": float(counted["saccades"].sum() / a.samples),
        "JSD_lattice_closed_vs_sampled_bits": M.jensen_shannon(exact["E"][0], counted["counts"][0]),
        "W1_amplitude_closed_vs_sampled_pixels": M.wasserstein_amplitude(exact["E"][0], counted["counts"][0], frame),
        "mean_amplitude_pixels": {"closed_form": s_exact["mean_amplitude"], "sampled": s_counted["mean_amplitude"]},
        "stay_share": {"closed_form": s_exact["stay"], "sampled": s_counted["stay"]},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
