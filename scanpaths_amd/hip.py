"""ctypes binding of libscanpaths_amd.so, derived at import from the C ABI declared in include/scanpaths_amd.h (_abi.py).

The product path has NO CPU fallback: if the shared library is missing or a tensor is not on a HIP
device, the calls raise.  torch is used only for device memory and the current stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _abi
from . import config as _config

_HERE = os.path.dirname(os.path.abspath(__file__))
# config library="timing" (tools/ only; SP_LIBRARY=timing under SP_ALLOW_ENV_TUNING=1): the A/B build with wrong-result timing modes
# compiled in (make -C scanpaths_amd/csrc timing).  The product path always loads libscanpaths_amd.so.
TIMING_LIB = False
LIB_PATH = ""


def _apply_config():
    global TIMING_LIB, LIB_PATH
    TIMING_LIB = _config.settings["library"] == "timing"
    LIB_PATH = os.path.join(_HERE, "libscanpaths_amd_timing.so" if TIMING_LIB else "libscanpaths_amd.so")


_apply_config()


# The binding is READ from the header, once, here: its integer defines, its two descriptor structs and every entry point
# (scanpaths_amd/_abi.py holds the rules and refuses what they do not cover).  SIGNATURES: name -> (restype, argtypes) in header order.
_DEFINES, _STRUCTS, SIGNATURES = _abi.load()
ConvDesc, WgradDesc = _STRUCTS["sp_conv_desc"], _STRUCTS["sp_wgrad_desc"]
ABI_VERSION = _DEFINES["SP_ABI_VERSION"]

_lib: Optional[C.CDLL] = None


def bind(cdll: C.CDLL, names=None) -> C.CDLL:
    """give the entry points `names` (default: all) of a loaded library the header's restype / argtypes"""
    for name in SIGNATURES if names is None else names:
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return cdll


def lib() -> C.CDLL:
    """Load the HIP library (once).  Raises loudly when it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  scanpaths_amd has no CPU or eager fallback.")
        _lib = bind(C.CDLL(LIB_PATH))
        if _lib.sp_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH}: ABI version {_lib.sp_abi_version()}, this binding expects {ABI_VERSION} (SP_ABI_VERSION in "
                               "include/scanpaths_amd.h; bumped whenever a descriptor layout or an entry point's meaning changes): rebuild "
                               "with `make -C scanpaths_amd/csrc`")
        # every max|.| slot this host passes comes zeroed from functional._amax_hint's pool and is used once: the launchers add
        # their reset node only while a stream is being captured (graph replays re-use the slot)
        if not _config.settings["always_reset_amax"]:
            check(_lib.sp_set_tuning(b"amax_reset", 1), "sp_set_tuning")
        if _lib.sp_timing_build() != int(TIMING_LIB):
            raise RuntimeError(f"{LIB_PATH}: timing / product build mix-up")
        if TIMING_LIB and _config.env_tuning_allowed():      # A/B timing / profiling knobs, honoured by the timing build only
            for env, knob in _config.TIMING_KNOBS.items():
                if os.environ.get(env):
                    check(_lib.sp_set_tuning(knob, int(os.environ[env])), "sp_set_tuning")
    return _lib


# The second library (include/scanpaths_amd_stats.h): the descriptive statistics that came after the main library's
# entry points were pinned.  Bound from its own header by the same rules; SIGNATURES, ABI_VERSION and lib() know nothing of it.
STATS_HEADER_PATH = os.path.join(os.path.dirname(_abi.HEADER_PATH), "scanpaths_amd_stats.h")
STATS_LIB_PATH = os.path.join(_HERE, "libscanpaths_amd_stats.so")
_STATS_DEFINES, _, STATS_SIGNATURES = _abi.load(STATS_HEADER_PATH)
STATS_ABI_VERSION = _STATS_DEFINES["SP_STATS_ABI_VERSION"]

_stats_lib: Optional[C.CDLL] = None


def _load_side_library(path, signatures, version_entry, version, define, header) -> C.CDLL:
    """a library beside the main one: every entry point typed from its header; a missing file or another ABI version raises"""
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C scanpaths_amd/csrc; hipcc --offload-arch=gfx950).  scanpaths_amd has no CPU or eager fallback.")
    cdll = C.CDLL(path)
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    found = getattr(cdll, version_entry)()
    if found != version:
        raise RuntimeError(f"{path}: ABI version {found}, this binding expects {version} "
                           f"({define} in include/{header}): rebuild with `make -C scanpaths_amd/csrc`")
    return cdll


def stats_lib() -> C.CDLL:
    """Load libscanpaths_amd_stats.so (once), every entry point typed from its header.  A missing file or another ABI version raises."""
    global _stats_lib
    if _stats_lib is None:
        _stats_lib = _load_side_library(STATS_LIB_PATH, STATS_SIGNATURES, "sp_stats_abi_version", STATS_ABI_VERSION,
                                        "SP_STATS_ABI_VERSION", "scanpaths_amd_stats.h")
    return _stats_lib


# The third library (include/scanpaths_amd_model.h): the model's statistics in closed form.  The stats library's exports
# are pinned as the main library's are; this one is where the next closed-form statistic goes, with its version bumped.
MODEL_HEADER_PATH = os.path.join(os.path.dirname(_abi.HEADER_PATH), "scanpaths_amd_model.h")
MODEL_LIB_PATH = os.path.join(_HERE, "libscanpaths_amd_model.so")
_MODEL_DEFINES, _, MODEL_SIGNATURES = _abi.load(MODEL_HEADER_PATH)
MODEL_ABI_VERSION = _MODEL_DEFINES["SP_MODEL_ABI_VERSION"]

_model_lib: Optional[C.CDLL] = None


def model_lib() -> C.CDLL:
    """Load libscanpaths_amd_model.so (once), every entry point typed from its header.  A missing file or another ABI version raises."""
    global _model_lib
    if _model_lib is None:
        _model_lib = _load_side_library(MODEL_LIB_PATH, MODEL_SIGNATURES, "sp_model_abi_version", MODEL_ABI_VERSION,
                                        "SP_MODEL_ABI_VERSION", "scanpaths_amd_model.h")
    return _model_lib


class HipError(RuntimeError):
    pass


def check(rc: int, what: str) -> None:
    if rc != 0:
        kind = {_DEFINES["SP_EINVAL"]: "SP_EINVAL (unsupported shape/alignment)",
                _DEFINES["SP_ENULL"]: "SP_ENULL (null pointer)"}.get(rc, f"hipError {rc}")
        raise HipError(f"{what} failed: {kind}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError("scanpaths_amd kernels need tensors on a HIP device (no CPU path)")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def device_index(device) -> int:
    """the ordinal of a torch device, the current one for a bare "cuda": the key of every per-device cache"""
    return device.index if device.index is not None else torch.cuda.current_device()


_side = {}


def side_stream(device) -> "torch.cuda.Stream":
    """one extra HIP stream per device: in the backward recurrence it carries the h-gate conv's data gradient of decode step t
    (functional._GateConvLstm.backward) beside the current stream's chain of small launches; the fan-in of h_{t-1}'s gradients
    (functional._FanOut.backward) waits for the event that launch leaves behind.  Deferred weight gradients run on the CURRENT stream."""
    key = device_index(device)
    s = _side.get(key)
    if s is None:
        # lowest priority the device offers (this pool's MI355X boxes: range (0, -1), i.e. normal): the side stream carries ONE long GEMM
        # beside the current stream's chain of small launches (A/B of normal vs high: 233.5 / 233.7 vs 233.6 / 234.6 ms per step)
        try:
            lo = max(torch.cuda.Stream.priority_range())
        except Exception:
            lo = 0
        s = torch.cuda.Stream(device=device, priority=lo)
        _side[key] = s
    return s


_ws = {}


def workspace(nbytes: int, device, slot: int = 0) -> Optional[torch.Tensor]:
    """Grow-only scratch buffer per (device, stream, slot); safe because the kernels of one stream run in order and a slot is consumed by
    the launch that requested it before the next request on that stream (round 5: one data gradient per decode step runs on the side
    stream beside the current one -- each stream has its own scratch)."""
    if nbytes <= 0:
        return None
    key = (device_index(device), torch.cuda.current_stream().cuda_stream, slot)
    cur = _ws.get(key)
    if cur is None or cur.numel() < nbytes:
        cur = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = cur
    return cur


class KernelTimer:
    """HIP-event timing of individual GEMM launches on the launch stream (bench.py roofline leg).
    Only launches with at least ``min_flops`` algorithmic FLOPs are bracketed, so the timed region is not perturbed
    by ~2000 extra event records per step."""

    def __init__(self, min_flops: float = 1e11):
        self.min_flops = min_flops
        self.pending = []          # (key, flops, start_event, end_event)

    def bracket(self, key, flops, launch):
        if flops < self.min_flops:
            return launch()
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        launch()
        e.record()
        # a launch enqueued on the side stream runs BESIDE the current stream's small launches: its time includes that contention and is
        # not comparable with a stand-alone launch of the same kernel -- the key says so ("+side"), bench.py reports it as `beside_chain`
        cur = torch.cuda.current_stream()
        sd = _side.get(device_index(cur.device))
        if sd is not None and cur.cuda_stream == sd.cuda_stream and isinstance(key, tuple) and key and isinstance(key[0], str):
            key = (key[0] + "+side",) + tuple(key[1:])
        self.pending.append((key, flops, s, e))

    def summary(self):
        """key -> dict(launches, flops_per_launch, avg_ms, tflops); call after a device synchronise."""
        out = {}
        for key, flops, s, e in self.pending:
            d = out.setdefault(key, {"launches": 0, "flops_per_launch": flops, "ms": 0.0})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
        for d in out.values():
            d["avg_ms"] = d["ms"] / d["launches"]
            d["tflops"] = d["flops_per_launch"] / (d["avg_ms"] * 1e-3) / 1e12
        return out


TIMER: Optional[KernelTimer] = None
