"""The device calls of the statistics that count into one array per group (saccade_statistics: a displacement lattice, turn_statistics:
a transition table), once for both: scanpaths that exist are counted by grouped_counts, the model's step distributions are summed in
closed form by grouped_expectation.  The callers have checked their own arguments; what is checked here needs the packed batch.  Both
C entry points take, between their scalars and their outputs, the caller's read-only tables (uploaded with the batch; tables() builds
them once there is something to launch) and then its extra scalars -- none for the lattice, the sector table and n_directions for the
turns.  A statistic of the second library (recurrence_statistics) names it with library=, a callable like _library below, and asks for
its further per-scanpath outputs with per_scanpath=; the defaults are the main library and none."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr
from . import _batch
from ._args import MAX_CELLS, MAX_DIRECTIONS, check_groups, rows


def _library():
    """the loaded library, its limits held to this side's: the one kernel-limit check of both statistics, or HipError"""
    L = hip.lib()
    _batch.check_limits(L)
    if L.sp_scan_likelihood_max_cells() != MAX_CELLS or L.sp_scan_turn_max_directions() != MAX_DIRECTIONS:
        raise hip.HipError(f"kernel limits {L.sp_scan_likelihood_max_cells()} / {L.sp_scan_turn_max_directions()}, this module expects "
                           f"{MAX_CELLS} / {MAX_DIRECTIONS}")
    return L


def grouped_counts(entry, device, scanpaths, groups, n_groups, frame, map_shape, max_steps, *, shape, unit, tables=dict, scalars=(),
                   library=None, per_scanpath=None) -> Dict[str, np.ndarray]:
    """entry(rows, ncol, starts, counts, group, S, G, max_steps, Hm, Wm, frame_w, frame_h, *tables, *scalars, counts, unit, dropped,
    *per_scanpath, stream) -> {"counts": int64 [G, *shape], unit: int32 [S], "dropped": int32 [S]} and, per name of per_scanpath
    {name: width}, int32 [S, width]; no scanpath: zeros, and no device is asked for"""
    b = _batch.pack([rows(sp)[:, :2] for sp in scanpaths], min_cols=2)
    S = len(b.counts)
    grp, G = check_groups(groups, S, n_groups, "scanpath")
    more = dict(per_scanpath or {})
    if S == 0:
        return {"counts": np.zeros((G,) + shape, np.int64), unit: np.zeros(0, np.int32), "dropped": np.zeros(0, np.int32),
                **{k: np.zeros((0, w), np.int32) for k, w in more.items()}}
    tables, dev, L = tables(), device(), (library or _library)()
    buf, at = _batch.upload(b.sections(group=grp, **tables), dev)
    out = _batch.Out({"counts": (np.int64, G * shape[0] * shape[1]), unit: (np.int32, S), "dropped": (np.int32, S),
                      **{k: (np.int32, S * w) for k, w in more.items()}}, dev)
    check(getattr(L, entry)(at["rows"], b.ncol, at["starts"], at["counts"], at["group"], S, G, max_steps, *map_shape, frame[1], frame[0],
                            *[at[k] for k in tables], *scalars, out.ptr("counts"), out.ptr(unit), out.ptr("dropped"),
                            *[out.ptr(k) for k in more], hip.stream()), entry)
    host = out.host()
    return dict(host, counts=host["counts"].reshape((G,) + shape), **{k: host[k].reshape(S, w) for k, w in more.items()})


def grouped_expectation(entry, device, probs, map_shape, row_groups, n_groups, min_length, max_steps, *, shape, work, name, unit,
                        tables=dict, scalars=(), library=None) -> Dict[str, np.ndarray]:
    """entry(probs, row_group, R, T, Hm, Wm, G, min_length, max_steps, *tables, *scalars, work, name, unit, bad, stream), work: scratch
    of that many doubles -> {name: float64 [G, *shape], unit: float64 [R], "bad": int32 [R]}; probs: checked, still as the caller's"""
    R, T, _ = probs.shape
    grp, G = check_groups(row_groups, R, n_groups, "row")
    tables, dev, L = tables(), device(), (library or _library)()
    buf, at = _batch.upload(dict(row_group=grp, **tables), dev)
    p = probs.detach().to(torch.float32).contiguous()
    scratch = torch.empty(work, dtype=torch.float64, device=dev)
    out = _batch.Out({name: (np.float64, G * shape[0] * shape[1]), unit: (np.float64, R), "bad": (np.int32, R)}, dev)
    check(getattr(L, entry)(ptr(p), at["row_group"], R, T, *map_shape, G, min_length, max_steps, *[at[k] for k in tables], *scalars,
                            ptr(scratch), out.ptr(name), out.ptr(unit), out.ptr("bad"), hip.stream()), entry)
    host = out.host()
    return dict(host, **{name: host[name].reshape((G,) + shape)})
