"""SED and STDE with the reference's interface (utils/evaltools/visual_attention_metrics.py:300-318, :392-441), computed by
csrc/scanmetrics.hip, plus the batched form the validation loops need:

    sed  = string_edit_distance(stimulus, human_scanpath, simulated_scanpath)                 # int
    stde = scaled_time_delay_embedding_similarity(human_scanpath, simulated_scanpath, stimulus)   # float, None if a path is empty
    sed, stde = sed_stde_pairs(scanpaths, pairs, stimulus.shape)                                  # device tensors [npairs]

    auc, nss, kld = saliency_metrics_pairs(saliency_maps, fixation_maps)                        # device tensors [N]
    maps, dropped = fixation_maps(scanpaths, groups, frame_size)                                 # saliency_maps.py, re-exported here
    dens = density_maps(maps, sigma=10)
    scores = scanpath_saliency(gt_scanpaths, gt_groups, pred_scanpaths, pred_groups, frame_size, sigma=10)
    extra = saliency_scores_pairs(saliency_maps, fixation_maps, density_maps, baseline_maps, image_groups=img, uniform_mix=0.01)
    # {"sAUC", "CC", "SIM", "IG": device tensors [N]}; per map: AUC_shuffled, CC, SIM, InfoGain

    d = scanpath_distances_pairs(scanpaths, pairs, metrics=("DTW", "REC", "DET"), radius=30.0)   # {metric: float64 numpy [npairs]}
    DTW(h, s), frechet_distance(h, s), hausdorff_distance(h, s), eyenalysis_distance(h, s), cross_recurrence(h, s, radius=30.0)

    lik = scanpath_likelihood(probs, scanpaths, rows, frame_size, uniform_mix=0.01)              # scanpath_likelihood.py, re-exported here:
    # {"LL", "NSS", "AUC": float64 numpy [S, T], "n", "dropped"}: human fixations under the model's own step distributions

SED is bit-exact; STDE follows numpy's float64 evaluation order (differences only in the last bit of exp()).  No CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr
from . import _batch
from ._batch import MAX_FIXATIONS  # noqa: F401  (re-exported)


def _device() -> torch.device:
    return _batch.device("scanpath metrics run")


def _on_device(batch, pairs):
    """what a pairwise scorer needs once its refusals are over: (device, library with its limits checked, the one upload of the
    scanpaths and pairs: buffer and {name: address})"""
    dev = _device()
    L = hip.lib()
    _batch.check_limits(L)
    return (dev, L) + _batch.upload(batch.sections(pairs=pairs), dev)


def sed_stde_pairs(scanpaths: Sequence[np.ndarray], pairs, image_shape, n: int = 5, want_sed: bool = True, want_stde: bool = True
                   ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """scanpaths: list of [n_k, >=2] arrays (x, y, ...), empty ones allowed; pairs: int [npairs, 2] = (human index, simulated index);
    image_shape: shape of the stimulus (height, width[, channels]).  Returns (sed int32 [npairs], stde float64 [npairs]); with an
    empty scanpath SED is the other one's length and STDE is NaN."""
    b = _batch.pack(scanpaths, min_cols=2)
    pr = _batch.check_pairs(pairs, len(b.counts))
    npairs = len(pr)
    dev, L, buf, at = _on_device(b, pr)
    sed = torch.empty(npairs, dtype=torch.int32, device=dev) if want_sed else None
    stde = torch.empty(npairs, dtype=torch.float64, device=dev) if want_stde else None
    if npairs:
        check(L.sp_scan_sed_stde(at["rows"], b.ncol, at["starts"], at["counts"], at["pairs"], npairs, int(image_shape[0]),
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


def _count_positive(f_d) -> np.ndarray:
    """the fixated-pixel counts (F > 0) of device rows [N,P]: one device reduction and one [N] copy"""
    cnt = torch.empty(f_d.shape[0], dtype=torch.int32, device=f_d.device)
    check(hip.lib().sp_count_positive(ptr(f_d), f_d.shape[0], f_d.shape[1], ptr(cnt), hip.stream()), "sp_count_positive")
    return cnt.cpu().numpy().astype(np.int64)


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
            nfix = _count_positive(f_d)
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


# ---- shuffled AUC, CC, SIM, information gain (Bylinskii et al., TPAMI 2019; no counterpart in the reference), csrc/salmaps.hip --------
# The paper's formulae on SUM-normalised maps.  The MATLAB benchmark code additionally min-max normalises a map before SIM and IG;
# that is not done here, because it changes a density's likelihood.
EXTRA_METRICS = ("sAUC", "CC", "SIM", "IG")


def _is_device_f64(m) -> bool:
    return isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float64


def _host_or_device(m):
    """a float64 device tensor as it is, anything else as a float64 numpy array"""
    if m is None or _is_device_f64(m):
        return m
    return np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float64)


def _rows_on_device(m, N, P, dev):
    if m is None:
        return None
    if isinstance(m, torch.Tensor):
        return m.contiguous().reshape(N, P)
    return torch.from_numpy(np.ascontiguousarray(m.reshape(N, P))).to(dev)


def _check_mix(uniform_mix) -> float:
    if uniform_mix is None:
        raise TypeError("information gain needs the keyword uniform_mix (the weight of the uniform density mixed into both maps; it has "
                        "no default: 0 is allowed, and then every fixation on an exact zero of a density costs 52 bits)")
    a = float(uniform_mix)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"uniform_mix {uniform_mix!r}: a weight in [0, 1]")
    return a


def _scratch_offsets(nfix: np.ndarray, lds: int, dev):
    """sp_saliency_scores' scratch slices: 8 * next_pow2(Nfix) bytes for a map with more fixated pixels than the LDS holds"""
    need = np.zeros(len(nfix), dtype=np.int64)
    big = nfix > lds
    if big.any():
        need[big] = 8 * 2 ** np.ceil(np.log2(nfix[big])).astype(np.int64)
    off = np.zeros(len(nfix) + 1, dtype=np.int64)
    off[1:] = np.cumsum(need)
    return torch.from_numpy(off).to(dev), (torch.empty(int(off[-1]), dtype=torch.uint8, device=dev) if off[-1] else None)


def _pool_counts_device(f_d, cls: np.ndarray, E: int):
    """sp_fixation_pool_counts of device rows [G,P]: (cls on the device [G], cnt [E,P], tot [P]) int32"""
    G, P = f_d.shape
    dev = f_d.device
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    cls_d = torch.empty(G, dtype=torch.int32, device=dev)
    cnt = torch.empty((E, P), dtype=torch.int32, device=dev)
    tot = torch.empty(P, dtype=torch.int32, device=dev)
    check(hip.lib().sp_fixation_pool_counts(ptr(f_d), cls.ctypes.data, G, P, E, ptr(cls_d), ptr(cnt), ptr(tot), hip.stream()),
          "sp_fixation_pool_counts")
    return cls_d, cnt, tot


def _saliency_scores_device(s_d, f_d=None, d_d=None, b_d=None, pool=None, pool_stride=0, cnt=None, cls_d=None, E=0, uniform_mix=0.0,
                            nfix=None, want=EXTRA_METRICS) -> Dict[str, torch.Tensor]:
    """sp_saliency_scores on contiguous float64 device rows [N,P]: ONE launch for the metrics of `want` whose inputs are given"""
    L = hip.lib()
    dev = s_d.device
    N, P = s_d.shape
    have = {"sAUC": f_d is not None and pool is not None, "CC": d_d is not None, "SIM": d_d is not None,
            "IG": f_d is not None and b_d is not None}
    out = {m: torch.empty(N, dtype=torch.float64, device=dev) for m in EXTRA_METRICS if m in want and have[m]}
    if not out:
        return out
    off_d = scratch = None
    if "sAUC" in out:
        off_d, scratch = _scratch_offsets(_count_positive(f_d) if nfix is None else nfix, L.sp_saliency_metrics_lds_fixations(), dev)
    check(L.sp_saliency_scores(ptr(s_d), ptr(f_d), ptr(d_d), ptr(b_d), ptr(pool) if "sAUC" in out else None, pool_stride, ptr(cnt),
                               ptr(cls_d), E, N, P, float(uniform_mix), ptr(off_d), ptr(scratch), ptr(out.get("sAUC")),
                               ptr(out.get("CC")), ptr(out.get("SIM")), ptr(out.get("IG")), hip.stream()), "sp_saliency_scores")
    return out


def saliency_scores_pairs(saliency_maps, fixation_maps=None, density_maps=None, baseline_maps=None, other_maps=None, image_groups=None,
                          *, uniform_mix=None) -> Dict[str, torch.Tensor]:
    """Shuffled AUC, CC, SIM and information gain of N maps, [N,H,W] each (numpy or torch; float64 device tensors are used in place,
    anything else is computed in float64), from one launch per entry point whatever N.  Returns a dict of float64 device tensors [N]
    with the metrics the inputs allow:
      "sAUC": fixation_maps (fixated where > 0) and the negatives' pool, given either as other_maps [N,H,W] (non-negative integer
              weights per pixel) or as image_groups [N] (the image each map was recorded on: the pool of map g is then every pixel
              fixated in a map of ANOTHER image, weighted by the number of such maps).  The exact weighted Mann-Whitney AUC of the
              unnormalised saliency values: ties count half, no random splits, no threshold step.
      "CC", "SIM": density_maps.  Pearson correlation; sum of min(S / sum S, D / sum D).
      "IG": fixation_maps and baseline_maps, and the keyword uniform_mix (required then, no default; 0 is allowed): the mean over the
              fixated pixels of log2(eps + p) - log2(eps + q), p = (1 - uniform_mix) S / sum S + uniform_mix / (H W), q the same of the
              baseline, eps = 2^-52.
    These are the paper's formulae (Bylinskii et al. 2019) on sum-normalised maps; the MATLAB benchmark code's additional min-max
    normalisation before SIM and IG is not applied, because it changes a density's likelihood.  NaN: sAUC without a fixation, with
    an empty pool or a NaN pixel; CC of a constant map; SIM / IG with a sum <= 0 or not finite; IG without a fixation.  No resizing:
    mismatched shapes raise."""
    maps = {"saliency": _host_or_device(saliency_maps), "fixation": _host_or_device(fixation_maps),
            "density": _host_or_device(density_maps), "baseline": _host_or_device(baseline_maps)}
    S = maps["saliency"]
    if S.ndim != 3:
        raise ValueError(f"saliency maps {tuple(S.shape)}: [N,H,W] is required")
    for name, m in maps.items():
        if m is not None and tuple(m.shape) != tuple(S.shape):
            raise ValueError(f"{name} maps {tuple(m.shape)} and saliency maps {tuple(S.shape)}: the same [N,H,W] shape is required (no "
                             "resizing)")
    N, P = S.shape[0], S.shape[1] * S.shape[2]
    if other_maps is not None and image_groups is not None:
        raise ValueError("the pool of negatives comes from other_maps or from image_groups, not both")
    if (other_maps is not None or image_groups is not None) and maps["fixation"] is None:
        raise ValueError("the shuffled AUC needs fixation_maps")
    if maps["baseline"] is not None and maps["fixation"] is None:
        raise ValueError("information gain needs fixation_maps")
    alpha = _check_mix(uniform_mix) if maps["baseline"] is not None else 0.0
    cls = E = other = None
    if image_groups is not None:
        cls = np.asarray(image_groups.cpu() if isinstance(image_groups, torch.Tensor) else list(image_groups), dtype=np.int64).reshape(-1)
        if cls.shape[0] != N or (N and cls.min() < 0):
            raise ValueError(f"image_groups: {N} non-negative image indices are required, got {cls.shape[0]}")
        E = int(cls.max()) + 1 if N else 0
    if other_maps is not None:
        other = other_maps if isinstance(other_maps, torch.Tensor) else np.asarray(other_maps)
        if tuple(other.shape) != tuple(S.shape):
            raise ValueError(f"other maps {tuple(other.shape)} and saliency maps {tuple(S.shape)}: the same [N,H,W] shape is required")
        if isinstance(other, torch.Tensor):
            o = other.to(torch.float64)
            bad = (~torch.isfinite(o) | (o != o.round()) | (o < 0) | (o > 2 ** 31 - 1)).any()
        else:
            o = other.astype(np.float64)
            bad = not np.isfinite(o).all() or (o != np.round(o)).any() or (o < 0).any() or (o > 2 ** 31 - 1).any()
        if bool(bad):
            raise ValueError("other maps hold counts: non-negative integers are required")
    if not any(m is not None for m in (other, cls, maps["density"], maps["baseline"])):
        raise ValueError("nothing to score: give a pool (other_maps or image_groups), density_maps or baseline_maps")
    dev = _device()
    if N == 0:
        empty = {"sAUC": maps["fixation"] is not None and (other is not None or cls is not None), "CC": maps["density"] is not None,
                 "SIM": maps["density"] is not None, "IG": maps["baseline"] is not None}
        return {m: torch.empty(0, dtype=torch.float64, device=dev) for m in EXTRA_METRICS if empty[m]}
    s_d, f_d, d_d, b_d = (_rows_on_device(maps[k], N, P, dev) for k in ("saliency", "fixation", "density", "baseline"))
    F = maps["fixation"]
    nfix = None if F is None or isinstance(F, torch.Tensor) else (F.reshape(N, -1) > 0).sum(1).astype(np.int64)
    if other is not None:
        pool = (other if isinstance(other, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(other))).to(device=dev, dtype=torch.int32)
        return _saliency_scores_device(s_d, f_d, d_d, b_d, pool.contiguous().reshape(N, P), P, uniform_mix=alpha, nfix=nfix)
    if cls is not None:
        cls_d, cnt, tot = _pool_counts_device(f_d, cls, E)
        return _saliency_scores_device(s_d, f_d, d_d, b_d, tot, 0, cnt, cls_d, E, alpha, nfix)
    return _saliency_scores_device(s_d, f_d, d_d, b_d, uniform_mix=alpha, nfix=nfix)


def AUC_shuffled(saliencyMap, fixationMap, otherMap):
    """Shuffled AUC (Zhang et al. 2008; Bylinskii et al. 2019) in its exact form: the weighted Mann-Whitney AUC of the saliency values
    at the fixated pixels (fixationMap > 0) against the pixels of otherMap, which holds non-negative integer counts (how often a pixel
    was fixated on OTHER images); ties count half, the map is compared unnormalised.  NaN without a fixation, with an empty otherMap
    or a NaN pixel; a non-integral or negative otherMap raises ValueError."""
    s, f = _pair(saliencyMap, fixationMap)
    _pair(saliencyMap, otherMap)
    return float(saliency_scores_pairs(s[None], f[None], other_maps=np.asarray(otherMap)[None])["sAUC"].item())


def CC(saliencyMap, densityMap):
    """Pearson's correlation coefficient of the two maps (NaN if one of them is constant)"""
    s, d = _pair(saliencyMap, densityMap)
    return float(saliency_scores_pairs(s[None], density_maps=d[None])["CC"].item())


def SIM(saliencyMap, densityMap):
    """histogram intersection of the two sum-normalised maps (no min-max step; NaN if a map's sum is <= 0 or not finite)"""
    s, d = _pair(saliencyMap, densityMap)
    return float(saliency_scores_pairs(s[None], density_maps=d[None])["SIM"].item())


def InfoGain(saliencyMap, fixationMap, baselineMap, *, uniform_mix):
    """information gain over the baseline in bits per fixation: mean over the fixated pixels of log2(eps + p) - log2(eps + q) with
    p = (1 - uniform_mix) S / sum S + uniform_mix / P, q the same of the baseline, eps = 2^-52 (sum-normalised maps, no min-max
    step).  uniform_mix is required: with 0 a fixation on an exact zero of a density costs 52 bits."""
    _check_mix(uniform_mix)
    s, f = _pair(saliencyMap, fixationMap)
    _, b = _pair(saliencyMap, baselineMap)
    return float(saliency_scores_pairs(s[None], f[None], baseline_maps=b[None], uniform_mix=uniform_mix)["IG"].item())


# ---- scanpath distances (visual_attention_metrics.py:205-218, :332-388, :444-476) ----------------------------------------------------
def tde_pairs(scanpaths: Sequence[np.ndarray], pairs, k: int = 0, distance_mode: str = 'Mean', max_dim: float = 1.0,
              want_euclidean: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """scanpaths / pairs as for sed_stde_pairs.  k >= 1: time_delay_embedding_distance(human / max_dim, simulated / max_dim, k,
    distance_mode); k == 0: the scaled distance over every k.  Returns (tde float64 [npairs], euclidean float64 [npairs] or None); NaN
    where the reference returns False / None."""
    if distance_mode not in ('Mean', 'Hausdorff'):
        raise ValueError(f"distance_mode {distance_mode!r}")
    b = _batch.pack(scanpaths, min_cols=2)
    pr = _batch.check_pairs(pairs, len(b.counts))
    npairs = len(pr)
    dev, L, buf, at = _on_device(b, pr)
    tde = torch.empty(npairs, dtype=torch.float64, device=dev)
    eucl = torch.empty(npairs, dtype=torch.float64, device=dev) if want_euclidean else None
    if npairs:
        check(L.sp_scan_tde(at["rows"], b.ncol, at["starts"], at["counts"], at["pairs"], npairs, int(k),
                            int(distance_mode == 'Hausdorff'), float(max_dim), ptr(tde), ptr(eucl), hip.stream()), "sp_scan_tde")
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


# ---- DTW, Frechet, Hausdorff, Eyenalysis, cross-recurrence (no counterpart in the reference), csrc/scandist.hip ------------
SCANPATH_DISTANCES = ("DTW", "Frechet", "Hausdorff", "Eyenalysis", "REC", "DET", "LAM", "CORM")
_RECURRENCE = SCANPATH_DISTANCES[4:]


def _check_distance_args(metrics, max_dim, radius, min_line):
    """(metrics as a tuple, max_dim, radius or None, min_line), or the refusal -- before any device or library call"""
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    unknown = [m for m in metrics if m not in SCANPATH_DISTANCES]
    if unknown:
        raise ValueError(f"unknown scanpath distance {unknown[0]!r}: one of {SCANPATH_DISTANCES}")
    if len(set(metrics)) != len(metrics):
        raise ValueError(f"repeated scanpath distance in {metrics}")
    if not metrics:
        raise ValueError("no scanpath distance asked for")
    md = float(max_dim)
    if not (np.isfinite(md) and md > 0):
        raise ValueError(f"max_dim {max_dim!r}: a positive finite number")
    if isinstance(min_line, bool) or int(min_line) != min_line or int(min_line) < 2:
        raise ValueError(f"min_line {min_line!r}: an integer >= 2")
    rad = None
    if any(m in _RECURRENCE for m in metrics):
        if radius is None:
            raise TypeError("the cross-recurrence measures need the keyword radius (in the units left after the division by max_dim; it "
                            "has no default)")
        rad = float(radius)
        if not (np.isfinite(rad) and rad > 0):
            raise ValueError(f"radius {radius!r}: a positive finite number")
    return metrics, md, rad, int(min_line)


def scanpath_distances_pairs(scanpaths: Sequence[np.ndarray], pairs, metrics=SCANPATH_DISTANCES[:4], max_dim: float = 1.0, radius=None,
                             min_line: int = 2) -> Dict[str, np.ndarray]:
    """scanpaths / pairs as for sed_stde_pairs: pairs[p] = (human index P, simulated index Q); only x and y are read, divided by max_dim
    first.  metrics: any of SCANPATH_DISTANCES (default: the four distances) --
      "DTW": dynamic time warping, D[i][j] = min(D[i-1][j-1], D[i-1][j], D[i][j-1]) + d(i,j); "Frechet": the discrete Frechet distance,
      the same recursion with max in place of +; "Hausdorff": max(max_i min_j d, max_j min_i d); "Eyenalysis" (position only):
      (sum_i min_j d + sum_j min_i d) / max(n, m);
      "REC", "DET", "LAM", "CORM": the cross-recurrence measures of Anderson et al. (2015) in per cent, over the first N = min(n, m)
      fixations of each scanpath, two fixations recurrent when d <= radius (keyword radius, required then, in the units left after the
      division by max_dim) and lines counted from min_line points.
    Returns {metric: float64 numpy [npairs]}: NaN for a pair with an empty scanpath; DET / LAM / CORM NaN without a recurrent point,
    CORM NaN for N = 1.  One upload, one launch per entry point (sp_scan_distances, sp_scan_recurrence) and one copy back whatever the
    number of pairs; an empty pair list touches no device."""
    metrics, md, rad, min_line = _check_distance_args(metrics, max_dim, radius, min_line)
    b = _batch.pack(scanpaths, min_cols=2)
    pr = _batch.check_pairs(pairs, len(b.counts))
    npairs = len(pr)
    if npairs == 0:
        return {m: np.zeros(0, dtype=np.float64) for m in metrics}
    dev, L, buf, at = _on_device(b, pr)
    dist = [m for m in SCANPATH_DISTANCES[:4] if m in metrics]
    sections = {m: (np.float64, npairs) for m in dist}
    if rad is not None:
        sections["recurrence"] = (np.float64, 4 * npairs)
    out = _batch.Out(sections, dev)
    args = (at["rows"], b.ncol, at["starts"], at["counts"], at["pairs"], npairs, md)
    if dist:
        check(L.sp_scan_distances(*args, out.ptr("DTW"), out.ptr("Frechet"), out.ptr("Hausdorff"), out.ptr("Eyenalysis"), hip.stream()),
              "sp_scan_distances")
    if rad is not None:
        check(L.sp_scan_recurrence(*args, rad, min_line, out.ptr("recurrence"), hip.stream()), "sp_scan_recurrence")
    host = out.host()
    rec = host["recurrence"].reshape(npairs, 4) if rad is not None else None
    return {m: np.ascontiguousarray(rec[:, _RECURRENCE.index(m)]) if m in _RECURRENCE else host[m] for m in metrics}


def _one_distance(metric, human_scanpath, simulated_scanpath):
    return float(scanpath_distances_pairs([human_scanpath, simulated_scanpath], [(0, 1)], metrics=(metric,))[metric][0])


def DTW(human_scanpath, simulated_scanpath):
    """dynamic time warping distance of the two scanpaths' positions (sum of d along the cheapest monotone alignment); NaN if one is empty"""
    return _one_distance("DTW", human_scanpath, simulated_scanpath)


def frechet_distance(human_scanpath, simulated_scanpath):
    """discrete Frechet distance (Eiter & Mannila 1994): the largest d along the monotone alignment that keeps it smallest"""
    return _one_distance("Frechet", human_scanpath, simulated_scanpath)


def hausdorff_distance(human_scanpath, simulated_scanpath):
    """Hausdorff distance of the two sets of fixation positions"""
    return _one_distance("Hausdorff", human_scanpath, simulated_scanpath)


def eyenalysis_distance(human_scanpath, simulated_scanpath):
    """Eyenalysis (Mathot et al. 2012) on positions only: every fixation's distance to the nearest fixation of the other scanpath,
    summed over both scanpaths and divided by the longer one's length"""
    return _one_distance("Eyenalysis", human_scanpath, simulated_scanpath)


def cross_recurrence(human_scanpath, simulated_scanpath, *, radius, min_line=2):
    """{"REC", "DET", "LAM", "CORM"} of Anderson et al. (2015), in per cent: recurrence, determinism (diagonal lines), laminarity (row
    and column lines) and centre of recurrence mass of the cross-recurrence matrix of the first min(n, m) fixations.  radius (pixels;
    required, no default): two fixations are recurrent when d <= radius."""
    res = scanpath_distances_pairs([human_scanpath, simulated_scanpath], [(0, 1)], metrics=_RECURRENCE, radius=radius, min_line=min_line)
    return {m: float(res[m][0]) for m in _RECURRENCE}


from .saliency_maps import density_maps, fixation_maps, gaussian_weights, scanpath_saliency  # noqa: E402,F401  (producers of the maps above)
from .scanpath_likelihood import cell_baselines, scanpath_likelihood  # noqa: E402,F401  (human scanpaths under the model's distributions)
