"""Turn statistics at the size of a validation pass: two routes to the SAME direction-transition table for the same rows of step
distributions -- the closed form (evaltools/turn_statistics.turn_expectation: exact, no sampling noise) and the sampled route (10
samples per row through Sampling.random_sample / generate_scanpath, then turn_counts).  Workload: 600 rows x 16 steps x 1201 actions
(the 30 x 40 map on 240 x 320), 8 directions, min_length 1, max_steps 16.
    python tests/diagnostics/bench_turn_statistics.py [--rows 600] [--samples 10] [--reps 7] [--out profiles/bench_turn_statistics.json]
Both times are a host clock around the whole route, ending in the copy back that synchronises; the distributions are on the device
before the clock starts, as they are after a forward.  The closed form: the upload of the row groups and the sector table, the three
launches, one copy back of the table.  The sampled route: per sample one sp_sample_actions and two sp_generate_scanpath launches with
their copies and the host loop that builds the fixation vectors (what run_test_loop does), then ONE turn_counts call for all samples.
One warm-up of each route comes first; the timed repeats alternate the two routes, and the medians are reported next to every single
time.  The Jensen-Shannon divergences between the two tables are sanity figures: they are the sampling noise of rows x samples
scanpaths, not an error.  No speed bar is set: the closed form's case is exactness.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_turn_statistics.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_turn_statistics needs a HIP device: a time taken elsewhere says nothing")
    from scanpaths_amd.models.sampling import Sampling
    from scanpaths_amd.utils.evaltools import turn_statistics as M
    T, shape, frame, min_length, max_steps, n = 16, (30, 40), (240, 320), 1, 16, 8
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
        return M.turn_expectation(d_probs, groups, 1, min_length=min_length, max_steps=max_steps, frame_size=frame, n_directions=n,
                                  map_shape=shape)

    def sampled():
        fvs = []
        for _ in range(a.samples):
            s = sampler.random_sample(d_probs, d_mu, d_s2)
            fvs += sampler.generate_scanpath(images, s["selected_actions_probs"], s["durations"], s["selected_actions"])[0]
        return M.turn_counts(fvs, np.zeros(len(fvs), dtype=np.int64), 1, frame, shape, max_steps=max_steps, n_directions=n)

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
    s_exact, s_counted = M.turn_summary(exact["M"][0]), M.turn_summary(counted["counts"][0])
    cmp_ = M.turn_comparison(exact["M"][0], counted["counts"][0])
    triples = a.rows * (T - 2)
    rec = {
        "metric": "turn statistics of one validation-sized pass: two routes to one direction-transition table, seconds per route",
        "rows": a.rows, "steps": T, "actions": 1 + P, "map_shape": list(shape), "n_directions": n, "min_length": min_length,
        "max_steps": max_steps, "samples_per_row": a.samples, "sampled_scanpaths": int(len(counted["pairs"])),
        "kernel_shape": "turn_expectation: one 256-thread block per (row, step triple), three step maps in LDS as doubles, the sector table "
                        "as bytes, two fans [n + 1][256] per batch of 256 middle cells, one thread per table entry over the batch, then one "
                        "thread per (row, entry) and per (group, entry); turn_counts: one wavefront per scanpath, integer atomics "
                        "(csrc/scanturn.hip)",
        "turn_expectation_s": float(np.median(t_closed)), "turn_expectation_s_all": [float(t) for t in t_closed],
        "turn_expectation_s_min_max": [float(min(t_closed)), float(max(t_closed))],
        "sampled_route_s": float(np.median(t_sampled)), "sampled_route_s_all": [float(t) for t in t_sampled],
        "sampled_route_s_min_max": [float(min(t_sampled)), float(max(t_sampled))],
        "closed_form_is_faster": bool(np.median(t_closed) < np.median(t_sampled)),
        "device_kind": "host clock around each whole route, ending in the copy back that synchronises; routes alternate; one warm-up each",
        "closed_form_sector_lookups": int(triples * 2 * P * P),
        "closed_form_sector_lookups_per_s_whole_call": float(triples * 2 * P * P / np.median(t_closed)),
        "device_scratch_bytes": int(triples * (n + 1) ** 2 * 8), "bytes_copied_back_closed_form": int((n + 1) ** 2 * 8 + 12 * a.rows),
        "rows_bad": int((exact["bad"] != 0).sum()), "expected_pairs": float(exact["pairs"].sum()),
        "expected_pairs_table_total": float(exact["M"].sum()),
        "sampled_pairs_per_sample_of_all_rows": float(counted["pairs"].sum() / a.samples),
        "JSD_turn_closed_vs_sampled_bits": cmp_["JSD_turn"], "JSD_transition_closed_vs_sampled_bits": cmp_["JSD_transition"],
        "JSD_table_closed_vs_sampled_bits": M.jensen_shannon(exact["M"][0], counted["counts"][0]),
        "forward_share": {"closed_form": s_exact["forward"], "sampled": s_counted["forward"]},
        "reversal_share": {"closed_form": s_exact["reversal"], "sampled": s_counted["reversal"]},
        "persistence": {"closed_form": s_exact["persistence"], "sampled": s_counted["persistence"]},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
