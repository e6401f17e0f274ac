"""Human scanpaths under the model's step distributions, one validation-sized batch: scanpath_likelihood on the device against the host
path -- copy the distributions back, then run the numpy restatement (tests/scanpath_likelihood_ref.py with quick=True: numpy sums per
step, a Python loop over the fixations, one core).  Workload: 32 rows x 16 steps x 1201 actions (the 30 x 40 map), 15 subjects per row
with 3-16 fixations each in a 320x240 frame, all six metrics (IG against one centre-prior row), uniform_mix 0.01, min_length 2.
    python tests/diagnostics/bench_scanpath_likelihood.py [--rows 32] [--subjects 15] [--reps 5] [--out profiles/bench_scanpath_likelihood.json]
The device time is a host clock around the whole call: packing, the one upload, the one launch, the one copy back (which synchronises)
and the STOP sums on the host; the distributions are on the device before the clock starts, as they are after a forward.  One warm-up
call comes first.  The host time starts with the copy of the distributions to the host.  Prints one JSON line and writes it to --out."""
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


def workload(rows, subjects, T, A, g):
    z = g.normal(0, 3, (rows, T, A))
    e = np.exp(z - z.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    mu = g.normal(-1.2, 0.5, (rows, T)).astype(np.float32)
    s2 = g.uniform(0.05, 1.5, (rows, T)).astype(np.float32)
    paths, row = [], []
    for r in range(rows):
        for _ in range(subjects):
            n = int(g.integers(3, 17))
            paths.append(np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.08, 0.6, n)], 1))
            row.append(r)
    return probs, mu, s2, paths, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--subjects", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_scanpath_likelihood.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scanpath_likelihood needs a HIP device: a time taken elsewhere says nothing")
    import scanpath_likelihood_ref as R
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    from scanpaths_amd.utils.evaltools import scanpath_likelihood as M
    T, shape, frame, u, min_length = 16, (30, 40), (240, 320), 0.01, 2
    P = shape[0] * shape[1]
    g = np.random.Generator(np.random.PCG64(0))
    probs, mu, s2, paths, row = workload(a.rows, a.subjects, T, 1 + P, g)
    baseline = g.uniform(0.1, 1.0, (1, P))
    brows = np.zeros(len(paths), dtype=np.int64)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_probs, d_mu, d_s2, d_base = (torch.from_numpy(x).to(dev) for x in (probs, mu, s2, baseline))

    def device_call():
        return M.scanpath_likelihood(d_probs, paths, row, frame, uniform_mix=u, metrics=M.METRICS, map_shape=shape, baseline=d_base,
                                     baseline_rows=brows, log_normal_mu=d_mu, log_normal_sigma2=d_s2, min_length=min_length)

    def host_call():
        h_probs, h_mu, h_s2 = d_probs.cpu().numpy(), d_mu.cpu().numpy(), d_s2.cpu().numpy()
        return R.scanpath_likelihood(h_probs, paths, row, frame, shape, u, baseline, brows, h_mu, h_s2, min_length, quick=True)

    counts = {"launches": 0, "bytes_back": 0}
    L = hip.lib()
    launch, host = L.sp_scan_likelihood, _batch.Out.host

    def counted_launch(*args):
        counts["launches"] += 1
        return launch(*args)

    def counted_host(self, *names):
        counts["bytes_back"] += self.buf.numel()
        return host(self, *names)

    L.sp_scan_likelihood, _batch.Out.host = counted_launch, counted_host
    try:
        device_call()                                    # warm-up: code object, allocator
        counts.update(launches=0, bytes_back=0)
        res = device_call()
        per_call = dict(counts)
    finally:
        L.sp_scan_likelihood, _batch.Out.host = launch, host
    t_dev, t_host = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_call()
        t_dev.append(time.perf_counter() - t0)
    ref = None
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = host_call()
        t_host.append(time.perf_counter() - t0)
    worst = {}
    for m in M.METRICS:
        x, y = res[m], ref[m]
        fin = np.isfinite(y)
        same = np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~fin], y[~fin], equal_nan=True)
        worst[m] = float((np.abs(x[fin] - y[fin]) / np.maximum(1.0, np.abs(y[fin]))).max()) if same else None
    dev_s, host_s = float(np.median(t_dev)), float(np.median(t_host))
    rec = {
        "metric": "scanpath_likelihood of one validation-sized batch, all six metrics, seconds per call",
        "rows": a.rows, "steps": T, "actions": 1 + P, "subjects_per_row": a.subjects, "scanpaths": len(paths),
        "fixations_scored": int(res["n"].sum()), "uniform_mix": u, "min_length": min_length,
        "kernel_shape": "one wavefront per (row, step), four per 256-thread block; the step's map in 32 registers per lane (csrc/scanlik.hip)",
        "device_s": dev_s, "device_s_all": [float(t) for t in t_dev], "device_launches_per_call": per_call["launches"],
        "device_bytes_copied_back_per_call": per_call["bytes_back"],
        "device_kind": "host clock around the whole call: packing, one upload, one launch, one copy back (synchronises), STOP sums on the host",
        "host_s": host_s, "host_s_all": [float(t) for t in t_host],
        "host_bytes_copied_back_per_call": int(probs.nbytes + mu.nbytes + s2.nbytes),
        "host_kind": "copy probs / mu / sigma2 back, then tests/scanpath_likelihood_ref.py quick=True (numpy sums per step, a Python loop "
                     "over the fixations, one core)",
        "host_over_device": host_s / dev_s, "worst_relative_difference_host_vs_device": worst,
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}", "host_cpus_used": 1,
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
