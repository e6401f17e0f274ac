"""The bootstrap at the package's own scale: G = 2000 keys in C = 1000 clusters, M = 32 columns, S = 32 plain contrasts plus 16 paired
differences, B = 10 000 replicates, five quantiles -- one call of evaltools/bootstrap.bootstrap_ratio (csrc/scanboot.hip) next to the
vectorised numpy route a user would otherwise write on the host: rng.integers multiplicities through np.bincount, then a matrix product.
    python tests/diagnostics/bench_bootstrap.py [--reps 7] [--out profiles/bench_bootstrap.json]
bootstrap_ratio_s is a host clock around the whole call -- the sort by cluster, the chunk plan, the upload, every launch and the copy
back of the summary, which synchronises.  The per-launch times come from a separate pass with a pair of HIP events around every entry
point of the library (the events cost time of their own, so that pass is not the one the whole call is timed in).  The numpy route's
replicates come from another generator, so only the times and the standard errors are set side by side, not the bytes: the two sets of
standard errors differ by the bootstrap's own noise, about sqrt(1 / (2 B)) = 0.7 %.  One warm-up of each route comes first; the timed
repeats alternate the two routes, and the medians are reported next to every single time.  Kernel-only hardware counters are not taken.
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

QUANTILES = (0.0, 0.025, 0.5, 0.975, 1.0)


def workload(G, C, Mc, g):
    labels = np.concatenate([np.arange(C), g.integers(0, C, G - C)])[g.permutation(G)]
    value = g.normal(0.5, 0.2, (G, Mc)) + g.normal(0.0, 0.1, (C, 1))[labels]          # a shared per-image offset: the keys of an image agree
    value[g.random((G, Mc)) < 0.02] = np.nan                                            # a key without a score here and there
    contrasts = [(m, -1, -1, -1) for m in range(Mc)] + [(2 * m, 2 * m + 1, -1, -1) for m in range(Mc // 2)]
    return labels, value, np.array(contrasts)


def numpy_route(num, den, labels, contrasts, B, seed):
    """the host route: multiplicities by bincount, replicate sums by a matrix product"""
    C = int(labels.max()) + 1
    N = np.stack([np.bincount(labels, weights=num[:, m], minlength=C) for m in range(num.shape[1])], 1)
    D = np.stack([np.bincount(labels, weights=den[:, m], minlength=C) for m in range(num.shape[1])], 1)
    idx = np.random.default_rng(seed).integers(0, C, (B, C))
    W = np.bincount((idx + np.arange(B)[:, None] * C).ravel(), minlength=B * C).reshape(B, C).astype(np.float64)
    R = (W @ N) / (W @ D)
    stat = np.stack([R[:, i] - (R[:, j] if j >= 0 else 0.0) for i, j, _, _ in contrasts], 0)
    return {"se": stat.std(axis=1, ddof=1), "quantiles": np.quantile(stat, QUANTILES, axis=1, method="inverted_cdf").T}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_bootstrap.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bootstrap needs a HIP device: a time taken elsewhere says nothing")
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import bootstrap as M
    G, C, Mc, B, seed = 2000, 1000, 32, 10000, 1
    labels, value, contrasts = workload(G, C, Mc, np.random.Generator(np.random.PCG64(0)))
    num, den = np.where(np.isnan(value), 0.0, value), np.where(np.isnan(value), 0.0, 1.0)
    chunks = M.column_chunks(contrasts)

    def device():
        return M.bootstrap_ratio(num, den, labels, contrasts, replicates=B, seed=seed, quantiles=QUANTILES)

    def host():
        return numpy_route(num, den, labels, contrasts, B, seed)

    dres, hres = device(), host()                          # warm-up: code objects, allocator, BLAS threads
    t_dev, t_host = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dres = device()
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hres = host()
        t_host.append(time.perf_counter() - t0)

    # per launch: a pair of events around every entry point, in a pass of its own
    L = hip.lib()
    names = ("sp_boot_cluster_sums", "sp_boot_resample", "sp_boot_summarise")
    originals = {n: getattr(L, n) for n in names}
    events = []
    for n, fn in originals.items():
        def timed(*args, _n=n, _fn=fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rc = _fn(*args)
            e.record()
            events.append((_n, s, e))
            return rc
        setattr(L, n, timed)
    try:
        per_launch = {}
        for _ in range(a.reps):
            del events[:]
            device()
            torch.cuda.synchronize()
            seen = {}
            for n, s, e in events:
                k = seen[n] = seen.get(n, -1) + 1
                per_launch.setdefault(f"{n}[{k}]" if n == "sp_boot_resample" else n, []).append(s.elapsed_time(e) * 1e-3)
    finally:
        for n, fn in originals.items():
            setattr(L, n, fn)
    launches = {k: float(np.median(v)) for k, v in per_launch.items()}
    ratio = hres["se"] / dres["se"]
    rec = {
        "metric": "cluster bootstrap of one evaluation-sized score table, seconds per call: bootstrap_ratio on the device next to the "
                  "vectorised numpy route on the host",
        "keys": G, "clusters": C, "columns": Mc, "contrasts": int(len(contrasts)), "replicates": B, "quantiles": list(QUANTILES),
        "column_chunks": [int(len(c)) for c, _ in chunks],
        "kernel_shape": "cluster sums: one thread per (cluster, column); resample: one wavefront per replicate, Philox draws, lane-strided "
                        "float64 row sums of the [C, M] tables read from L2, xor butterfly, ratios and contrasts, at most 32 columns per "
                        "launch; summarise: one block per statistic for counts, mean and sd, one thread per replicate for its rank "
                        "(csrc/scanboot.hip)",
        "bootstrap_ratio_s": float(np.median(t_dev)), "bootstrap_ratio_s_all": [float(t) for t in t_dev],
        "numpy_route_s": float(np.median(t_host)), "numpy_route_s_all": [float(t) for t in t_host],
        "device_is_faster": bool(np.median(t_dev) < np.median(t_host)),
        "launch_s": launches, "launch_s_sum": float(sum(launches.values())),
        "device_kind": "whole call: host clock, ending in the copy back that synchronises; routes alternate; one warm-up each.  "
                       "Per launch: HIP events around each entry point of the library, median over the repeats of a separate pass.  "
                       "No hardware counters were taken",
        "draws_per_call": int(len(chunks) * (B + 1) * C), "row_reads_bytes": int(sum(len(c) for c, _ in chunks) * 2 * 8 * (B + 1) * C),
        "bytes_uploaded": int(2 * G * sum(len(c) for c, _ in chunks) * 8 + C * 12 + contrasts.size * 4 + len(QUANTILES) * 8),
        "bytes_copied_back": int(len(contrasts) * (3 * 8 + len(QUANTILES) * 8 + 3 * 4)),
        "n_valid_min": int(dres["n_valid"].min()),
        "se_device_first_columns": [float(v) for v in dres["se"][:4]], "se_numpy_first_columns": [float(v) for v in hres["se"][:4]],
        "se_ratio_numpy_over_device": {"min": float(ratio.min()), "median": float(np.median(ratio)), "max": float(ratio.max())},
        "box": f"{torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}, torch {torch.__version__}",
        "host_cpus_used": int(os.environ.get("OMP_NUM_THREADS", 0)) or None,
    }
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
