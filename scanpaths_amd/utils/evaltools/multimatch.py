"""MultiMatch (Dewhurst et al. 2012, Jarodzka et al. 2010) -- the five scanpath similarities the reference obtains from the
third-party ``multimatch_gaze.docomparison`` (utils/evaluation.py:8,43,213; multimatch_gaze==0.1.2, sp_baseline.yml:65).

That package is NOT vendored in the reference and is absent here, so this is a restatement of its published algorithm with the
reference's call arguments (screensize=[320, 240], no grouping / simplification): saccade vectors of both scanpaths -> matrix of
vector differences -> cheapest monotone alignment path from the first to the last saccade pair (steps right / down / diagonal,
cost = the entered cell) -> medians of the vector, direction, length, position and duration differences along the path ->
normalisation to [0, 1].  Scanpaths with fewer than 3 fixations give five NaNs (the rule that makes the reference drop a pair).
PARITY: **unpinned** -- no fixture of the original package exists in the reference; utils/evaluation.py uses the installed
``multimatch_gaze`` instead whenever it is importable.

Two forms: ``docomparison`` (host numpy, one pair; the reference's call signature) and ``multimatch_pairs`` (round 4: ALL pairs of a
validation call in one launch of ``sp_scan_multimatch``, one thread per pair -- the triple python loop per pair was the wall-clock of
validation once ScanMatch / SED / STDE ran on the device).  The host form is the device kernel's checker (tests/test_scanmatch_gpu.py).

Simplification (``grouping=True``) is MultiMatch's first stage: successive saccades that point the same way (angle
below TDir degrees) and successive short saccades (below TAmp pixels) are merged unless the fixation between them lasts TDur or
longer, until nothing changes.  Here it DELETES fixations: merging saccades i and i + 1 removes fixation i + 1, so the result is an
ordinary, shorter scanpath.  float64, every operation rounded on its own.  With n saccades, lx_i = x_{i+1} - x_i, ly_i likewise,
rho_i = sqrt(lx_i*lx_i + ly_i*ly_i), for 0 <= i <= n - 2:
  direction candidate  (lx_i*lx_{i+1} + ly_i*ly_{i+1}) > cosT * (rho_i * rho_{i+1})  and  duration_{i+1} < TDur, with cosT =
                       cos(radians(TDir)) computed once on the host (the device gets the same double); a zero-length saccade is never
                       one (0 > 0 is false); no direction pass at all for TDir == 0 (cosT >= 1)
  amplitude candidate  rho_i < TAmp  and  duration_{i+1} < TDur
One pass, either kind, is greedy and left to right on the arrays as they are at its start: a candidate i deletes fixation i + 1 and the
pass goes on at i + 2, otherwise at i + 1 (within a run of candidates those at even offset are taken).  One round = a direction pass,
then an amplitude pass on its result; rounds repeat until one deletes nothing.  The first and the last fixation are never deleted; a
path of fewer than 3 fixations is returned unchanged.  Scoring with grouping: five NaNs if either ORIGINAL scanpath has fewer than 3
fixations, otherwise the simplified paths are scored, even one of 2 fixations = 1 saccade.
``simplify_scanpath`` is the host restatement (plain loops) and the checker of ``simplify_scanpaths`` / ``sp_scan_simplify`` (one
wavefront per scanpath, all scanpaths of a call in one launch).  Known differences from ``multimatch_gaze`` (parity unpinned as above):
  * the special handling of the last saccade in its amplitude pass is not restated;
  * merged vectors are recomputed from the kept fixations rather than summed (equal up to rounding, exactly on integer grids)."""
from __future__ import annotations

import math

import numpy as np

from ... import hip
from ...hip import check
from . import _batch
from ._batch import MAX_FIXATIONS  # noqa: F401  (re-exported; one lane per fixation in sp_scan_simplify)


def _structure(data):
    a = np.array([list(_) for _ in list(data)], dtype=np.float64).reshape(-1, 3)
    x, y, dur = a[:, 0], a[:, 1], a[:, 2]
    lenx, leny = x[1:] - x[:-1], y[1:] - y[:-1]
    return {"fx": x, "fy": y, "dur": dur, "sx": x[:-1], "sy": y[:-1], "lenx": lenx, "leny": leny,
            "rho": np.sqrt(lenx ** 2 + leny ** 2), "theta": np.arctan2(leny, lenx)}


def _alignment(M):
    """cheapest path (0,0) -> (n-1,m-1) over moves right / down / diagonal, cost of a move = M at the cell entered"""
    n, m = M.shape
    D = np.full((n, m), np.inf)
    prev = np.zeros((n, m, 2), dtype=np.int64)
    D[0, 0] = 0.0
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                continue
            best, arg = np.inf, (0, 0)
            for di, dj in ((0, 1), (1, 0), (1, 1)):
                pi, pj = i - di, j - dj
                if pi >= 0 and pj >= 0 and D[pi, pj] + M[i, j] < best:
                    best, arg = D[pi, pj] + M[i, j], (pi, pj)
            D[i, j] = best
            prev[i, j] = arg
    path = [(n - 1, m - 1)]
    while path[-1] != (0, 0):
        i, j = path[-1]
        path.append((int(prev[i, j, 0]), int(prev[i, j, 1])))
    return path[::-1]


def _rows(data):
    """fixation records / sequences of (x, y, duration) -> float64 [n, 3]; a plain 2-D array keeps its (>= 3) columns"""
    if isinstance(data, np.ndarray) and data.dtype.names is None and data.ndim == 2:
        a = np.asarray(data, dtype=np.float64)
        if a.shape[1] < 3:
            raise ValueError(f"a scanpath needs the columns x, y, duration: {a.shape[1]} columns")
        return a
    return np.array([list(_) for _ in list(data)], dtype=np.float64).reshape(-1, 3)


def _thresholds(TDir, TDur, TAmp):
    """(cosT, TDur, TAmp) as floats; ValueError unless all three are finite and >= 0 and TDir <= 180 degrees"""
    try:
        tdir, tdur, tamp = float(TDir), float(TDur), float(TAmp)
    except (TypeError, ValueError):
        raise ValueError(f"TDir, TDur, TAmp must be numbers: {TDir!r}, {TDur!r}, {TAmp!r}") from None
    for name, v in (("TDir", tdir), ("TDur", tdur), ("TAmp", tamp)):
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"{name} must be finite and >= 0: {v}")
    if tdir > 180:
        raise ValueError(f"TDir is an angle in degrees in [0, 180]: {tdir}")
    return (1.0 if tdir == 0 else math.cos(math.radians(tdir))), tdur, tamp


def _simplify_pass(rows, kind, cosT, tdur, tamp):
    """one greedy left-to-right pass over the candidates of the rows as they are now -> the kept rows"""
    n = len(rows) - 1                                              # saccades
    lx = [rows[i + 1][0] - rows[i][0] for i in range(n)]
    ly = [rows[i + 1][1] - rows[i][1] for i in range(n)]
    rho = [math.sqrt(lx[i] * lx[i] + ly[i] * ly[i]) for i in range(n)]
    drop = set()
    i = 0
    while i <= n - 2:
        if kind == "direction":
            cand = (lx[i] * lx[i + 1] + ly[i] * ly[i + 1]) > cosT * (rho[i] * rho[i + 1])
        else:
            cand = rho[i] < tamp
        if cand and rows[i + 1][2] < tdur:
            drop.add(i + 1)
            i += 2
        else:
            i += 1
    return [r for k, r in enumerate(rows) if k not in drop]


def simplify_scanpath(fixation_vectors, TDir, TDur, TAmp):
    """MultiMatch simplification of one scanpath on the host (the definition in the module docstring, in plain loops): float64
    [k, 3] = the kept (x, y, duration) rows.  The checker of simplify_scanpaths."""
    cosT, tdur, tamp = _thresholds(TDir, TDur, TAmp)
    rows = [(float(r[0]), float(r[1]), float(r[2])) for r in _rows(fixation_vectors)]
    while len(rows) >= 3:                                          # every round that continues deletes a fixation
        before = len(rows)
        if cosT < 1.0:
            rows = _simplify_pass(rows, "direction", cosT, tdur, tamp)
        rows = _simplify_pass(rows, "amplitude", cosT, tdur, tamp)
        if len(rows) == before:
            break
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _similarities(p1, p2, screensize):
    M = np.sqrt((p1["lenx"][:, None] - p2["lenx"][None, :]) ** 2 + (p1["leny"][:, None] - p2["leny"][None, :]) ** 2)
    path = _alignment(M)
    vec, ang, ln, pos, dur = [], [], [], [], []
    for i, j in path:
        vec.append(math.sqrt((p1["lenx"][i] - p2["lenx"][j]) ** 2 + (p1["leny"][i] - p2["leny"][j]) ** 2))
        t = [p1["theta"][i], p2["theta"][j]]
        t = [math.pi + (math.pi + v) if v < 0 else v for v in t]
        d = abs(t[0] - t[1])
        ang.append(2 * math.pi - d if d > math.pi else d)
        ln.append(abs(p1["rho"][i] - p2["rho"][j]))
        pos.append(math.sqrt((p1["sx"][i] - p2["sx"][j]) ** 2 + (p1["sy"][i] - p2["sy"][j]) ** 2))
        dur.append(abs(p1["dur"][i] - p2["dur"][j]) / max(p1["dur"][i], p2["dur"][j]))
    un = [float(np.median(v)) for v in (vec, ang, ln, pos, dur)]
    diag = math.sqrt(screensize[0] ** 2 + screensize[1] ** 2)
    return [1 - un[0] / (2 * diag), 1 - un[1] / math.pi, 1 - un[2] / diag, 1 - un[3] / diag, 1 - un[4]]


def docomparison(fixation_vectors1, fixation_vectors2, screensize, grouping=False, TDir=0.0, TDur=0.0, TAmp=0.0):
    if grouping:
        _thresholds(TDir, TDur, TAmp)
    if not (len(fixation_vectors1) >= 3 and len(fixation_vectors2) >= 3):
        return [np.nan] * 5
    if grouping:                        # the rule above looked at the ORIGINAL paths; a simplified one may be down to one saccade
        fixation_vectors1 = simplify_scanpath(fixation_vectors1, TDir, TDur, TAmp)[:, :3]
        fixation_vectors2 = simplify_scanpath(fixation_vectors2, TDir, TDur, TAmp)[:, :3]
    return _similarities(_structure(fixation_vectors1), _structure(fixation_vectors2), screensize)


def _on_device(batch, **more):
    """after the refusals: (device, library with its limits checked, the one upload: buffer and {name: address})"""
    L = hip.lib()
    _batch.check_limits(L)
    dev = _batch.device("MultiMatch runs")
    return (dev, L) + _batch.upload(batch.sections(**more), dev)


def simplify_scanpaths(scanpaths, *, TDir, TDur, TAmp):
    """MultiMatch simplification of many scanpaths on the device (sp_scan_simplify, one wavefront per scanpath): one upload, one
    launch and one copy back whatever their number.  scanpaths: list of fixation records or [n, >= 3] arrays (x, y, duration, ...;
    further columns are not read), at most 64 fixations each.  Returns a list of float64 [k, 3] arrays, equal bit for bit to
    simplify_scanpath of each.  Bad thresholds and too long scanpaths are refused before the device or the library is touched; an
    empty list touches neither."""
    cosT, tdur, tamp = _thresholds(TDir, TDur, TAmp)
    b = _batch.pack([_rows(a) for a in scanpaths], min_cols=3)
    K = len(b.counts)
    if not K:
        return []
    dev, L, buf, at = _on_device(b)
    out = _batch.Out({"rows": (np.float64, 3 * len(b.rows)), "kept": (np.int32, K)}, dev)
    check(L.sp_scan_simplify(at["rows"], b.ncol, at["starts"], at["counts"], K, cosT, tdur, tamp, out.ptr("rows"), out.ptr("kept"),
                             hip.stream()), "sp_scan_simplify")
    host = out.host()
    rows = host["rows"].reshape(-1, 3)
    return [rows[s:s + k].copy() for s, k in zip(b.starts, host["kept"])]


def multimatch_pairs(scanpaths, pairs, screensize, grouping=False, TDir=0.0, TDur=0.0, TAmp=0.0):
    """MultiMatch of many pairs on the device.  scanpaths: list of fixation records / arrays (x, y, duration); pairs: [npairs, 2]
    indices into scanpaths (first, second argument of docomparison); screensize [width, height].  Returns float64 [npairs, 5]
    (numpy), five NaNs for a pair with a scanpath of fewer than 3 fixations.
    grouping: the scanpaths are simplified on the device first (sp_scan_simplify with TDir, TDur, TAmp) and the simplified buffer is
    scored in place by sp_scan_multimatch_gated with the original counts as the gate: no round trip through the host in between.
    Bad thresholds, a scanpath of more than 64 fixations and a pair index out of range are refused before the device or the library
    is touched; an empty pair list returns an empty array.  One upload and one copy back (the scores) either way."""
    if grouping:
        cosT, tdur, tamp = _thresholds(TDir, TDur, TAmp)
    b = _batch.pack([np.array([list(_) for _ in list(a)], dtype=np.float64).reshape(-1, 3) for a in scanpaths], min_cols=3)
    pr = _batch.check_pairs(pairs, len(b.counts))
    if len(pr) == 0:
        return np.zeros((0, 5))
    dev, L, buf, at = _on_device(b, pairs=pr)
    sections = {"scores": (np.float64, 5 * len(pr))}
    if grouping:                                          # the simplified rows and their counts stay on the device
        sections.update(rows=(np.float64, 3 * len(b.rows)), kept=(np.int32, len(b.counts)))
    out = _batch.Out(sections, dev)
    size = (float(screensize[0]), float(screensize[1]))
    if grouping:
        check(L.sp_scan_simplify(at["rows"], 3, at["starts"], at["counts"], len(b.counts), cosT, tdur, tamp, out.ptr("rows"),
                                 out.ptr("kept"), hip.stream()), "sp_scan_simplify")
        check(L.sp_scan_multimatch_gated(out.ptr("rows"), 3, at["starts"], out.ptr("kept"), at["counts"], at["pairs"], len(pr), *size,
                                         out.ptr("scores"), hip.stream()), "sp_scan_multimatch_gated")
    else:
        check(L.sp_scan_multimatch(at["rows"], 3, at["starts"], at["counts"], at["pairs"], len(pr), *size, out.ptr("scores"),
                                   hip.stream()), "sp_scan_multimatch")
    return out.host("scores")["scores"].reshape(-1, 5)
