"""The host-side plumbing every evaluation scorer shares: a list of ragged scanpaths becomes

    rows float64 [total, ncol] | starts int64 [K] | counts int32 [K] | whatever else the scorer needs (pairs int32 [P, 2], groups ...)

in ONE host buffer that is uploaded by ONE copy, and the results that go back to the host sit in ONE device buffer that is copied back
once.  Every section of either buffer starts at a multiple of 8 bytes and owns at least 8 bytes, whatever its dtype, its length (counts
and pairs are int32 and may be odd in number) and its place in the order: no caller relies on section order for alignment, and the
address of an empty section is still a valid one inside the buffer.

pack, check_index, check_pairs and sections are pure numpy: a scorer finishes its refusals with them before it asks for a device or the
library.  upload and Out take the device as an argument and never obtain one themselves.

Lifetime: the caller binds what upload / Out return to a local name until its last launch has been enqueued.  Every launch goes to
hip.stream(), torch's current stream, so releasing the buffers after the enqueue is safe under torch's stream-ordered caching
allocator -- also for the scorers that return device tensors without synchronising.  Never pass a temporary's data_ptr() to a launch."""
from __future__ import annotations

from itertools import compress
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from ... import hip

MAX_FIXATIONS = 64          # = sp_scan_max_fixations(), known here so that a refusal needs no library (held equal by the tests)


def device(what: str) -> torch.device:
    """the current HIP device; what: the subject and verb of the refusal, e.g. "ScanMatch runs" """
    if not torch.cuda.is_available():
        raise hip.HipError(f"scanpaths_amd {what} on a HIP device only (no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def check_limits(L, max_points: Optional[int] = None) -> None:
    """the loaded library agrees with MAX_FIXATIONS (and, where given, with the caller's mean-shift limit), or HipError"""
    if max_points is not None:
        if L.sp_scan_max_fixations() != MAX_FIXATIONS or L.sp_meanshift_max_points() != max_points:
            raise hip.HipError(f"kernel limits {L.sp_scan_max_fixations()} / {L.sp_meanshift_max_points()}, this module expects "
                               f"{MAX_FIXATIONS} / {max_points}")
    elif L.sp_scan_max_fixations() != MAX_FIXATIONS:
        raise hip.HipError(f"sp_scan_max_fixations() = {L.sp_scan_max_fixations()}, this module expects {MAX_FIXATIONS}")


def starts(counts) -> np.ndarray:
    """int64: the first row of every run of counts[k] consecutive rows"""
    return np.cumsum(counts, dtype=np.int64) - counts


class Batch(NamedTuple):
    rows: np.ndarray        # float64 [total, ncol], C-contiguous
    ncol: int
    counts: np.ndarray      # int32 [K]
    starts: np.ndarray      # int64 [K]: starts(counts)

    def sections(self, **more) -> Dict[str, np.ndarray]:
        """the sections of an upload, in the names every scorer uses"""
        return dict(rows=self.rows, starts=self.starts, counts=self.counts, **more)


def pack(scanpaths, *, min_cols: int, what: str = "scanpath", limit: Optional[int] = MAX_FIXATIONS, allow_empty: bool = True) -> Batch:
    """list of [n, >= min_cols] arrays -> Batch.  An empty scanpath has no width of its own; ncol is the width of the non-empty ones
    (min_cols if there is none)."""
    arrs = [np.asarray(a, dtype=np.float64) for a in scanpaths]
    counts = np.array(list(map(len, arrs)), dtype=np.int32)
    if not allow_empty and len(counts) and counts.min() == 0:
        raise ValueError(f"{what} {int(counts.argmin())} is empty: every {what} needs a fixation")
    if limit is not None and len(counts) and counts.max() > limit:
        raise ValueError(f"{what} of {counts.max()} fixations exceeds the kernel limit {limit}")
    columns = ValueError(f"{what}s need the same number (>= {min_cols}) of columns")
    try:                                                      # numpy checks that the widths agree
        rows = np.concatenate(list(compress(arrs, counts)) or [np.zeros((0, min_cols))], 0)
    except ValueError:
        raise columns from None
    if rows.ndim != 2:                                        # flat scanpaths: one column
        rows = rows.reshape(len(rows), -1)
    if rows.shape[1] < min_cols:
        raise columns
    return Batch(rows, rows.shape[1], counts, starts(counts))


def check_index(values, n: int, what: str) -> np.ndarray:
    """values as int64, every one of them in [0, n), or ValueError"""
    v = np.asarray(values, dtype=np.int64)
    if v.size and (v.min() < 0 or v.max() >= n):
        raise ValueError(f"{what} index out of range: {n} to choose from, indices {v.min()} .. {v.max()}")
    return v


def check_pairs(pairs, n: int) -> np.ndarray:
    """pairs as C-contiguous int32 [P, 2], every index in [0, n), or ValueError"""
    return np.ascontiguousarray(check_index(pairs, n, "pair").reshape(-1, 2), dtype=np.int32)


def upload(sections: Dict[str, np.ndarray], dev):
    """the named host arrays in one buffer (module docstring), one copy to dev -> (the buffer: keep it, {name: address on dev})"""
    parts, off, pos = [], {}, 0
    for name, a in sections.items():
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        off[name] = pos
        pad = -len(b) % 8 if len(b) else 8
        parts += [b, np.zeros(pad, dtype=np.uint8)]
        pos += len(b) + pad
    buf = torch.from_numpy(np.concatenate(parts)).to(dev)
    return buf, {name: buf.data_ptr() + o for name, o in off.items()}


class Out:
    """the results of a call in one buffer on dev; sections: {name: (dtype, number of elements)}, laid out as the module docstring says"""

    def __init__(self, sections, dev):
        self.at, pos = {}, 0
        for name, (dtype, n) in sections.items():
            self.at[name] = (pos, np.dtype(dtype), n)
            pos += max((np.dtype(dtype).itemsize * n + 7) // 8 * 8, 8)
        self.buf = torch.empty(pos, dtype=torch.uint8, device=dev)

    def ptr(self, name) -> Optional[int]:
        """the address of a section; None for one that was not asked for"""
        return self.buf.data_ptr() + self.at[name][0] if name in self.at else None

    def host(self, *names) -> Dict[str, np.ndarray]:
        """{name: array} of the named sections (default: all) from ONE copy back of the bytes they span; synchronises"""
        at = {k: self.at[k] for k in names} if names else self.at
        lo = min((o for o, _, _ in at.values()), default=0)
        hi = max((o + dt.itemsize * n for o, dt, n in at.values()), default=0)
        raw = self.buf[lo:hi].cpu().numpy()
        return {name: raw[o - lo:o - lo + dt.itemsize * n].view(dt).copy() for name, (o, dt, n) in at.items()}
