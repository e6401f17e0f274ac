"""SED and STDE with the reference's interface (utils/evaltools/visual_attention_metrics.py:300-318, :392-441), computed by
csrc/scanmetrics.hip, plus the batched form the validation loops need:

    sed  = string_edit_distance(stimulus, human_scanpath, simulated_scanpath)                 # int
    stde = scaled_time_delay_embedding_similarity(human_scanpath, simulated_scanpath, stimulus)   # float, None if a path is empty
    sed, stde = sed_stde_pairs(scanpaths, pairs, stimulus.shape)                                  # device tensors [npairs]

    auc, nss, kld = saliency_metrics_pairs(saliency_maps, fixation_maps)                        # device tensors [N]
    maps, dropped = fixation_maps(scanpaths, groups, frame_size)                                 # saliency_maps.py, re-exported here
    dens = density_maps(maps, sigma=10)
    scores = scanpath_saliency(gt_scanpaths, gt_groups, pred_scanpaths, pred_groups, frame_size, sigma=10)

SED is bit-exact; STDE follows numpy's float64 evaluation order (differences only in the last bit of exp()).  No CPU path."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise hip.HipError("scanpaths_amd scanpath metrics run on a HIP device only (no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def sed_stde_pairs(scanpaths: Sequence[np.ndarray], pairs, image_shape, n: int = 5, want_sed: bool = True, want_stde: bool = True
                   ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """scanpaths: list of [n_k, >=2] arrays (x, y, ...); pairs: int [npairs, 2] = (human index, simulated index);
    image_shape: shape of the stimulus (height, width[, channels]).  Returns (sed int32 [npairs], stde float64 [npairs])."""
    dev = _device()
    L = hip.lib()
    arrs = [np.asarray(a, dtype=np.float64).reshape(len(a), -1) for a in scanpaths]
    ncol = arrs[0].shape[1]
    if any(a.shape[1] != ncol for a in arrs) or ncol < 2:
        raise ValueError("scanpaths need the same number (>= 2) of columns")
    counts = [a.shape[0] for a in arrs]
    if max(counts) > L.sp_scan_max_fixations():
        raise ValueError(f"scanpath of {max(counts)} fixations exceeds the kernel limit {L.sp_scan_max_fixations()}")
    count = torch.tensor(counts, dtype=torch.int32)
    start = (torch.cumsum(count.to(torch.int64), 0) - count.to(torch.int64)).to(dev)
    cat = np.concatenate(arrs, 0)
    if cat.shape[0] == 0:
        cat = np.zeros((1, ncol))
    fix = torch.from_numpy(cat).to(dev)
    pr = torch.as_tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(dev).contiguous()
    npairs = pr.shape[0]
    sed = torch.empty(npairs, dtype=torch.int32, device=dev) if want_sed else None
    stde = torch.empty(npairs, dtype=torch.float64, device=dev) if want_stde else None
    count_d = count.to(dev)          # named: must outlive the launch
    if npairs:
        check(L.sp_scan_sed_stde(ptr(fix), ncol, ptr(start), ptr(count_d), ptr(pr), npairs, int(image_shape[0]),
                                 int(image_shape[1]), int(n), float(max(image_shape)), ptr(sed), ptr(stde), hip.stream()),
              "sp_scan_sed_stde")
    return sed, stde


def string_edit_distance(stimulus, human_scanpath, simulated_scanpath, n=5, substitution_cost=1, msg=False):
    # substitution_cost is accepted and ignored, as in the reference (:317 calls _Levenshtein without it)
    sed, _ = sed_stde_pairs([human_scanpath, simulated_scanpath], [(0, 1)], np.shape(stimulus), n=n, want_stde=False)
    return int(sed.item())


def scaled_time_delay_embedding_similarity(human_scanpath, simulated_scanpath, image, toPlot=False, msg=False):
    if len(human_scanpath) == 0 or len(simulated_scanpath) == 0:
        return None
    _, stde = sed_stde_pairs([human_scanpath, simulated_scanpath], [(0, 1)], np.shape(image), want_sed=False)
    return float(stde.item())


# ---- saliency-map metrics (visual_attention_metrics.py:41-192), csrc/salmaps.hip ----------------------------------------------------
def saliency_metrics_pairs(saliency_maps, fixation_maps, jitter=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """saliency_maps, fixation_maps: [N,H,W] (numpy or torch; computed in float64), jitter: None or [N,H,W] added to the saliency maps
    before AUC-Judd's normalisation.  Returns device float64 tensors (auc_judd, nss, kldiv) of shape [N] from ONE launch -- the
    reference's AUC_Judd(s, f, jitter=False) / NSS(s, f) / KLdiv(s, f) per map, or AUC_Judd's jittered score when that map's jitter
    is given.  NaN where the reference returns NaN (no fixation; a constant map under AUC-Judd)."""
    dev = _device()
    on_device = all(isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float64 for m in (saliency_maps, fixation_maps))
    if on_device:                                                  # the maps stay where they are (saliency_maps.py produces them there)
        S, F = saliency_maps, fixation_maps
    else:
        S = np.asarray(saliency_maps.cpu() if isinstance(saliency_maps, torch.Tensor) else saliency_maps, dtype=np.float64)
        F = np.asarray(fixation_maps.cpu() if isinstance(fixation_maps, torch.Tensor) else fixation_maps, dtype=np.float64)
    if S.ndim != 3 or S.shape != F.shape:
        raise ValueError(f"saliency maps {tuple(S.shape)} and fixation maps {tuple(F.shape)}: the same [N,H,W] shape is required (no "
                         "resizing)")
    N, P = S.shape[0], S.shape[1] * S.shape[2]
    if N == 0:
        return tuple(torch.empty(0, dtype=torch.float64, device=dev) for _ in range(3))
    if on_device:
        s_d, f_d = S.contiguous().reshape(N, P), F.contiguous().reshape(N, P)
    else:
        s_d = torch.from_numpy(np.ascontiguousarray(S.reshape(N, P))).to(dev)
        f_d = torch.from_numpy(np.ascontiguousarray(F.reshape(N, P))).to(dev)
    j_d = None
    if jitter is not None:
        J = jitter if isinstance(jitter, torch.Tensor) else np.asarray(jitter, dtype=np.float64)
        if tuple(J.shape) != tuple(S.shape):
            raise ValueError(f"jitter {tuple(J.shape)} must have the saliency maps' shape {tuple(S.shape)}")
        if isinstance(J, torch.Tensor):
            j_d = J.to(device=dev, dtype=torch.float64).contiguous().reshape(N, P)
        else:
            j_d = torch.from_numpy(np.ascontiguousarray(J.reshape(N, P))).to(dev)
    return _saliency_metrics_device(s_d, f_d, j_d, None if on_device else (F.reshape(N, -1) > 0).sum(1))


def _saliency_metrics_device(s_d, f_d, j_d=None, nfix=None, want_auc=True):
    """sp_saliency_metrics on contiguous float64 device rows [N,P].  nfix: the fixated-pixel counts when the host has them, else they
    come from one device reduction and one [N] copy.  want_auc False gives no map a scratch slice: a map with more fixated pixels than
    the LDS holds then reports NaN for AUC-Judd without sorting them (NSS and KLdiv are unaffected)."""
    L = hip.lib()
    dev = s_d.device
    N, P = s_d.shape
    out = tuple(torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
    # AUC-Judd keeps the sorted fixated values in LDS up to sp_saliency_metrics_lds_fixations(); a map with more gets a slice of a
    # global scratch buffer: 8 * next_pow2(Nfix) + 4 * Nfix bytes (rounded up to 8)
    need = np.zeros(N, dtype=np.int64)
    if want_auc:
        if nfix is None:
            cnt = torch.empty(N, dtype=torch.int32, device=dev)
            check(L.sp_count_positive(ptr(f_d), N, P, ptr(cnt), hip.stream()), "sp_count_positive")
            nfix = cnt.cpu().numpy().astype(np.int64)
        lds = L.sp_saliency_metrics_lds_fixations()
        big = nfix > lds
        if big.any():
            n2 = 2 ** np.ceil(np.log2(np.maximum(nfix[big], 1))).astype(np.int64)
            need[big] = 8 * n2 + (4 * nfix[big] + 7) // 8 * 8
    off = np.zeros(N + 1, dtype=np.int64)
    off[1:] = np.cumsum(need)
    off_d = torch.from_numpy(off).to(dev)
    scratch = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev) if off[-1] else None
    check(L.sp_saliency_metrics(ptr(s_d), ptr(f_d), ptr(j_d), N, P, ptr(off_d), ptr(scratch), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                hip.stream()), "sp_saliency_metrics")
    return out


def _pair(saliencyMap, fixationMap):
    s, f = np.asarray(saliencyMap), np.asarray(fixationMap)
    if np.shape(s) != np.shape(f) or s.ndim != 2:
        raise ValueError(f"saliency map {np.shape(s)} and fixation map {np.shape(f)}: equal 2-D shapes are required (the reference's "
                         "interpolating resize of a mismatched map is not provided)")
    return s, f


def AUC_Judd(saliencyMap, fixationMap, jitter=True, toPlot=False, msg=False):
    """the reference's AUC_Judd (:41-118).  The jitter is drawn on the host exactly as the reference draws it
    (np.random.random(shape) / 10**7, only when there is a fixation), so the same np.random.seed gives the same score."""
    if toPlot:
        raise NotImplementedError("AUC_Judd(toPlot=True): plotting is not provided")
    s, f = _pair(saliencyMap, fixationMap)
    if not f.any():
        if msg:
            print('Error: no fixationMap')
        return float('nan')
    j = np.random.random(np.shape(s)) / 10 ** 7 if jitter else None
    if (f > 0).all():
        # every pixel fixated: the reference divides a Python float by the integer Npixels - Nfixations = 0 (:97) unless its
        # normalised map is all NaN (:78) -- raise as it does; the batched call returns the IEEE result instead
        sj = s.astype(float) + (0.0 if j is None else j)
        with np.errstate(all="ignore"):
            if not np.isnan((sj - sj.min()) / (sj.max() - sj.min())).all():
                raise ZeroDivisionError("float division by zero")
    auc, _, _ = saliency_metrics_pairs(s[None], f[None], None if j is None else j[None])
    score = float(auc.item())
    if msg and np.isnan(score):
        print('NaN saliencyMap')
    return score


def NSS(saliencyMap, fixationMap, msg=False):
    """the reference's NSS (:162-192): max-normalised, standardised with std(ddof=1), mean at the non-zero fixation pixels"""
    s, f = _pair(saliencyMap, fixationMap)
    if not f.any():
        if msg:
            print('Error: no fixationMap')
        return float('nan')
    _, nss, _ = saliency_metrics_pairs(s[None], f[None])
    return float(nss.item())


def KLdiv(saliencyMap, fixationMap):
    """the reference's KLdiv (:130-153), eps = 1e-12"""
    s, f = _pair(saliencyMap, fixationMap)
    _, _, kld = saliency_metrics_pairs(s[None], f[None])
    return float(kld.item())


# ---- scanpath distances (visual_attention_metrics.py:205-218, :332-388, :444-476) ----------------------------------------------------
def tde_pairs(scanpaths: Sequence[np.ndarray], pairs, k: int = 0, distance_mode: str = 'Mean', max_dim: float = 1.0,
              want_euclidean: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """scanpaths / pairs as for sed_stde_pairs.  k >= 1: time_delay_embedding_distance(human / max_dim, simulated / max_dim, k,
    distance_mode); k == 0: the scaled distance over every k.  Returns (tde float64 [npairs], euclidean float64 [npairs] or None); NaN
    where the reference returns False / None."""
    dev = _device()
    L = hip.lib()
    if distance_mode not in ('Mean', 'Hausdorff'):
        raise ValueError(f"distance_mode {distance_mode!r}")
    arrs = [np.asarray(a, dtype=np.float64) for a in scanpaths]
    arrs = [a.reshape(len(a), -1) if len(a) else np.zeros((0, a.shape[-1] if a.ndim == 2 else 2)) for a in arrs]
    ncol = max(a.shape[1] for a in arrs)
    if any(a.shape[1] != ncol and a.shape[0] > 0 for a in arrs) or ncol < 2:
        raise ValueError("scanpaths need the same number (>= 2) of columns")
    arrs = [a if a.shape[0] else np.zeros((0, ncol)) for a in arrs]
    counts = [a.shape[0] for a in arrs]
    if max(counts) > L.sp_scan_max_fixations():
        raise ValueError(f"scanpath of {max(counts)} fixations exceeds the kernel limit {L.sp_scan_max_fixations()}")
    count = torch.tensor(counts, dtype=torch.int32)
    start = (torch.cumsum(count.to(torch.int64), 0) - count.to(torch.int64)).to(dev)
    cat = np.concatenate(arrs, 0)
    if cat.shape[0] == 0:
        cat = np.zeros((1, ncol))
    fix = torch.from_numpy(cat).to(dev)
    pr = torch.as_tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(dev).contiguous()
    npairs = pr.shape[0]
    tde = torch.empty(npairs, dtype=torch.float64, device=dev)
    eucl = torch.empty(npairs, dtype=torch.float64, device=dev) if want_euclidean else None
    count_d = count.to(dev)          # named: must outlive the launch
    if npairs:
        check(L.sp_scan_tde(ptr(fix), ncol, ptr(start), ptr(count_d), ptr(pr), npairs, int(k), int(distance_mode == 'Hausdorff'),
                            float(max_dim), ptr(tde), ptr(eucl), hip.stream()), "sp_scan_tde")
    return tde, eucl


def euclidean_distance(human_scanpath, simulated_scanpath, msg=False):
    if len(human_scanpath) != len(simulated_scanpath):
        if msg:
            print('Error: The two sequences must have the same length!')
        return False
    if len(human_scanpath) == 0:
        return 0.0
    _, e = tde_pairs([human_scanpath, simulated_scanpath], [(0, 1)], k=1, want_euclidean=True)
    return float(e.item())


def time_delay_embedding_distance(human_scanpath, simulated_scanpath, k=3, distance_mode='Mean', msg=False):
    if len(human_scanpath) < k or len(simulated_scanpath) < k:
        if msg:
            print('ERROR: Too large value for the time-embedding vector dimension')
        return False
    if distance_mode not in ('Mean', 'Hausdorff'):
        if msg:
            print('ERROR: distance mode not defined.')
        return False
    if int(k) < 1:
        raise ValueError(f"time-embedding vector dimension k={k}: k >= 1 is required")
    tde, _ = tde_pairs([human_scanpath, simulated_scanpath], [(0, 1)], k=int(k), distance_mode=distance_mode)
    return float(tde.item())


def scaled_time_delay_embedding_distance(human_scanpath, simulated_scanpath, image, toPlot=False, msg=False):
    if len(human_scanpath) == 0 or len(simulated_scanpath) == 0:
        return None
    tde, _ = tde_pairs([human_scanpath, simulated_scanpath], [(0, 1)], k=0, max_dim=float(max(np.shape(image))))
    return float(tde.item())


from .saliency_maps import density_maps, fixation_maps, gaussian_weights, scanpath_saliency  # noqa: E402,F401  (producers of the maps above)
