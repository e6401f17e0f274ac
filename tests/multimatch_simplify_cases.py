"""Inputs shared by tests/test_multimatch_simplify_cpu.py and tests/test_multimatch_simplify_gpu.py: seeded random
scanpaths (half on a 40 x 30 lattice of 8 px with durations {1..6} * 0.1, where direction and amplitude decisions tie; half uniform),
the constructed cases whose simplification is written out by hand, and the argument lists of the two C entry points."""

import numpy as np

THRESHOLDS = (45.0, 0.3, 40.0)            # the usual setting on a 320 x 240 screen: 45 degrees, 0.3 s, 10 % of the diagonal
NEW = {"sp_scan_simplify": ("int", 11), "sp_scan_multimatch_gated": ("int", 11)}


def lattice_path(rng, n):
    a = np.zeros((n, 3))
    a[:, 0], a[:, 1], a[:, 2] = rng.integers(0, 40, n) * 8.0, rng.integers(0, 30, n) * 8.0, rng.integers(1, 7, n) * 0.1
    return a


def uniform_path(rng, n):
    a = np.zeros((n, 3))
    a[:, 0], a[:, 1], a[:, 2] = rng.uniform(0, 320, n), rng.uniform(0, 240, n), rng.uniform(0.05, 0.6, n)
    return a


def random_paths(seed, number, lengths=None):
    """(lattice paths, uniform paths), `number` of each; lengths 1 .. 64 unless given (then cycled through)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for make in (lattice_path, uniform_path):
        out.append([make(rng, int(rng.integers(1, 65)) if lengths is None else lengths[k % len(lengths)]) for k in range(number)])
    return out


def walk(n, duration=0.1):
    """n collinear fixations 8 px apart"""
    return np.array([[8.0 * i, 0.0, duration] for i in range(n)]).reshape(-1, 3)


def staircase(n, duration=0.1):
    """right-angle staircase of 8 px steps: right, up, right, ..."""
    return np.array([[8.0 * ((i + 1) // 2), 8.0 * (i // 2), duration] for i in range(n)]).reshape(-1, 3)


def run_case(k, closed=True):
    """k saccades of 8 px along x, then (closed) one of 100 px: with TAmp = 10 the first k are one run of amplitude candidates"""
    xs = [8.0 * i for i in range(k + 1)] + ([8.0 * k + 100.0] if closed else [])
    return np.array([[x, 0.0, 0.1] for x in xs])


# name -> (path, (TDir, TDur, TAmp), indices of the rows that stay), every one worked out by hand from the definition
_STAIR_LONG = staircase(7)
_STAIR_LONG[3, 2] = 0.5
CONSTRUCTED = {
    # amplitude pass, three rounds: {F1, F4} go, then {F2, F5}; F3 lasts 0.5 and stays
    "staircase amplitude 40": (_STAIR_LONG, (0.0, 0.3, 40.0), [0, 3, 6]),
    # the same first round; then the merged saccades are 11.3 px >= 10 and the 8 px one ends at the long fixation
    "staircase amplitude 10": (_STAIR_LONG, (0.0, 0.3, 10.0), [0, 2, 3, 5, 6]),
    # runs of 1 .. 4 candidates: the ones at even offset are taken (fixation offset + 1 goes); merged saccades are 16 px >= 10
    "run of 1": (run_case(1), (0.0, 0.3, 10.0), [0, 2]),
    "run of 2": (run_case(2), (0.0, 0.3, 10.0), [0, 2, 3]),
    "run of 3": (run_case(3), (0.0, 0.3, 10.0), [0, 2, 4]),
    "run of 4": (run_case(4), (0.0, 0.3, 10.0), [0, 2, 4, 5]),
    # a run that reaches the last saccade: the last fixation is no candidate's "next" fixation
    "open run of 2": (run_case(2, closed=False), (0.0, 0.3, 10.0), [0, 2]),
    "open run of 3": (run_case(3, closed=False), (0.0, 0.3, 10.0), [0, 2, 3]),
    "everything merges": (staircase(9), (180.0, 1e9, 1e9), [0, 8]),
    # 0 > cosT * 0 is false whatever cosT: a zero-length saccade is never direction-merged
    "zero saccade 180": (np.array([[0.0, 0.0, 0.1], [0.0, 0.0, 0.1], [8.0, 0.0, 0.1]]), (180.0, 1.0, 0.0), [0, 1, 2]),
    "zero saccade 45": (np.array([[0.0, 0.0, 0.1], [8.0, 0.0, 0.1], [8.0, 0.0, 0.1], [16.0, 0.0, 0.1]]), (45.0, 1.0, 0.0), [0, 1, 2, 3]),
    "right angles": (staircase(12), (45.0, 0.3, 0.0), list(range(12))),
    "long fixations": (walk(33, 0.5), (45.0, 0.3, 0.0), list(range(33))),
    "walk 33": (walk(33), (45.0, 0.3, 0.0), [0, 32]),
    "walk 64": (walk(64), (45.0, 0.3, 0.0), [0, 63]),
}


def check_refusals(lib):
    """SP_ENULL (-2) / SP_EINVAL (-1) of the two entry points: returned before anything is enqueued, so without a device too"""
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")
    simplify = [p, 3, p, p, 1, 0.5, 0.3, 40.0, p, p, None]
    assert all(lib.sp_scan_simplify(*[None if i == k else a for i, a in enumerate(simplify)]) == -2 for k in (0, 2, 3, 8, 9))
    for k, bad in ((4, 0), (4, -1), (1, 2), (1, 0), (5, 1.5), (5, -1.5), (5, nan), (6, -0.1), (6, nan), (6, inf), (7, -1.0), (7, nan),
                   (7, inf)):
        assert lib.sp_scan_simplify(*[bad if i == k else a for i, a in enumerate(simplify)]) == -1, (k, bad)
    gated = [p, 3, p, p, p, p, 1, 320.0, 240.0, p, None]
    assert all(lib.sp_scan_multimatch_gated(*[None if i == k else a for i, a in enumerate(gated)]) == -2 for k in (0, 2, 3, 4, 5, 9))
    for k, bad in ((6, 0), (6, -4), (1, 2), (7, 0.0), (8, -1.0), (7, nan)):
        assert lib.sp_scan_multimatch_gated(*[bad if i == k else a for i, a in enumerate(gated)]) == -1, (k, bad)
