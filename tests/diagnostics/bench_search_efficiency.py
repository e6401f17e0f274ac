"""Target-search efficiency at the size of a validation pass: the two device calls of evaltools/search_efficiency.py against the
plain-loop checker (tests/search_efficiency_ref.py, Python floats, one core) -- the only other implementation there is, so the ratio says
how long the check takes, not how fast a tuned host path would be.  Workload: 600 rows x 16 steps x 1201 actions (the 30 x 40 map) with
3 boxes per row for target_hit_probability, min_length 1; 4000 scanpaths of 1-12 fixations in a 320x240 frame, one box each, max_steps 6
for target_hits.
    python tests/diagnostics/bench_search_efficiency.py [--rows 600] [--boxes 3] [--scanpaths 4000] [--reps 5] [--out profiles/bench_search_efficiency.json]
The device times are a host clock around each whole call: packing, the one upload, the one launch and the one copy back (which
synchronises); the distributions are on the device before the clock starts, as they are after a forward.  One warm-up call of each comes
first.  The checker's time starts with the copy of the distributions to the host and is taken once.  Prints one JSON line and writes it
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=600)
    ap.add_argument("--boxes", type=int, default=3)
    ap.add_argument("--scanpaths", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_search_efficiency.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_search_efficiency needs a HIP device: a time taken elsewhere says nothing")
    import search_efficiency_ref as R
    from scanpaths_amd.utils.evaltools import search_efficiency as M
    T, shape, frame, min_length, max_steps = 16, (30, 40), (240, 320), 1, 6
    P = shape[0] * shape[1]
    g = np.random.Generator(np.random.PCG64(0))
    dev = torch.device("cuda", torch.cuda.current_device())
    z = torch.from_numpy(g.normal(0, 3, (a.rows, T, 1 + P)).astype(np.float32)).to(dev)
    d_probs = torch.softmax(z, 2)

    def box():
        w, h = g.uniform(20, 160), g.uniform(20, 120)
        x, y = g.uniform(0, frame[1] - w), g.uniform(0, frame[0] - h)
        return (x, y, x + w, y + h)

    boxes = np.array([box() for _ in range(a.rows * a.boxes)])
    box_rows = np.repeat(np.arange(a.rows), a.boxes)
    paths = [np.stack([g.uniform(0, frame[1], n), g.uniform(0, frame[0], n)], 1) for n in g.integers(1, 13, a.scanpaths)]
    path_boxes = np.array([box() for _ in paths])

    def mass():
        return M.target_hit_probability(d_probs, boxes, box_rows, frame, min_length=min_length, map_shape=shape)

    def hits():
        return M.target_hits(paths, path_boxes, max_steps=max_steps)

    got_mass, got_hits = mass(), hits()                      # warm-up: code object, allocator
    t_mass, t_hits = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mass()
        t_mass.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hits()
        t_hits.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want_mass = R.target_mass(d_probs.cpu().numpy(), boxes, box_rows, frame, shape, min_length)
    c_mass = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_hits = R.target_hits(paths, path_boxes, max_steps)
    c_hits = time.perf_counter() - t0
    equal = {k: bool(np.array_equal(got_mass[k], want_mass[k], equal_nan=True)) for k in got_mass}
    equal.update({k: bool(np.array_equal(got_hits[k], want_hits[k], equal_nan=True)) for k in got_hits})
    curve = M.search_curve(got_hits["hit"], max_steps)
    rec = {
        "metric": "search efficiency of one validation-sized pass, seconds per call",
        "rows": a.rows, "steps": T, "actions": 1 + P, "boxes_per_row": a.boxes, "boxes": int(len(boxes)), "min_length": min_length,
        "scanpaths": len(paths), "fixations": int(sum(len(p) for p in paths)), "max_steps": max_steps,
        "kernel_shape": "target_hit_probability: one 256-thread block per box, waves take steps round-robin, one lane runs the recursion; "
                        "target_hits: one wavefront per scanpath, four per block (csrc/scansearch.hip)",
        "target_hit_probability_s": float(np.median(t_mass)), "target_hit_probability_s_all": [float(t) for t in t_mass],
        "target_hits_s": float(np.median(t_hits)), "target_hits_s_all": [float(t) for t in t_hits],
        "device_kind": "host clock around each whole call: packing, one upload, one launch, one copy back (synchronises)",
        "bytes_copied_back": {"target_hit_probability": int(3 * 8 * len(boxes) * T + 4 * len(boxes)), "target_hits": int(20 * len(paths))},
        "checker_target_mass_s": float(c_mass), "checker_target_hits_s": float(c_hits),
        "checker_kind": "copy probs back, then tests/search_efficiency_ref.py (plain Python loops over IEEE doubles, one core), taken once",
        "bit_equal_to_checker": equal,
        "mean_model_tfp_at_last_step": float(np.nanmean(got_mass["TFP"][:, max_steps - 1])), "sampled_curve": [float(v) for v in curve],
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
