"""Fixation and density maps from scanpaths, on the device (csrc/fixmaps.hip): the producers of the inputs of saliency_metrics_pairs.

    maps, dropped = fixation_maps(scanpaths, groups, frame_size, output_shape=None, weight="binary")   # [G,H,W] float64, [G] int32
    dens = density_maps(maps, sigma, truncate=4.0, mode="constant", normalise=None)                    # scipy gaussian_filter per map
    scores = scanpath_saliency(gt_scanpaths, gt_groups, pred_scanpaths, pred_groups, frame_size, sigma)
    # {"AUC_Judd", "NSS", "KLdiv": float64 [G], "gt_dropped", "pred_dropped": int32 [G]}, all on the device
    scores = scanpath_saliency(..., extra_metrics=("sAUC", "CC", "SIM", "IG"), image_groups=img, uniform_mix=0.01)   # + those keys
    res = expected_fixation_maps(probs, row_groups, n_groups, min_length=1, max_steps=16, frame_size=(240, 320))     # the model, exactly
    # {"maps": float64 [G,H,W] on the device, "fixations": float64 [R], "bad": int32 [R]}  (csrc/scanexpect.hip)
    scores = scanpath_saliency(gt_scanpaths, gt_groups, [], [], frame_size, sigma, prediction="maps", pred_maps=res["maps"])

The reference has no such code (its callers rasterise with numpy and blur with scipy on the host); the pixel rule is the one of
include/scanpaths_amd.h sp_fixation_maps, the filter is scipy.ndimage.gaussian_filter.  sigma has no default: the library does not
pick a visual angle.  No interpolating resize of mismatched maps, no CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import hip
from ...hip import check, ptr
from . import _batch
from ._args import MAX_CELLS, check_frame, check_groups, check_map, check_map_shape, check_min_length, check_steps
from ._args import rows as _rows
from ._batch import MAX_FIXATIONS

WEIGHTS = {"binary": 0, "count": 1, "duration": 2}
MODES = {"constant": 0, "reflect": 1, "nearest": 2}
NORMALISE = {None: 0, "sum": 1, "max": 2}


def _device() -> torch.device:
    return _batch.device("fixation / density maps run")


class _Upload:
    """the concatenated fixations of a list of scanpaths with their start / count / group in one buffer on the device (ONE upload):
    fix, start, count and group are the device addresses of its sections, valid while the object lives"""

    def __init__(self, scanpaths: Sequence, groups, num_groups: Optional[int], dev):
        grp = np.asarray(list(groups), dtype=np.int64).reshape(-1)
        if len(scanpaths) != grp.shape[0]:
            raise ValueError(f"{len(scanpaths)} scanpaths but {grp.shape[0]} groups")
        if grp.size and grp.min() < 0:
            raise ValueError("negative group index")
        self.G = int(num_groups) if num_groups is not None else (int(grp.max()) + 1 if grp.size else 0)
        if grp.size and grp.max() >= self.G:
            raise ValueError(f"group index {int(grp.max())} with num_groups = {self.G}")
        b = _batch.pack([_rows(s) for s in scanpaths], min_cols=2, limit=None)
        self.ncol, self.K = b.ncol, len(b.counts)
        self._buf, at = _batch.upload(b.sections(group=grp.astype(np.int32)), dev)
        self.fix, self.start, self.count, self.group = at["rows"], at["starts"], at["counts"], at["group"]

    def rasterise(self, frame_size, output_shape, weight: str, K: Optional[int] = None, G: Optional[int] = None):
        """maps [G,H,W], dropped [G] of the first K scanpaths (all by default)"""
        if weight not in WEIGHTS:
            raise ValueError(f"weight {weight!r}: one of {sorted(WEIGHTS)}")
        if weight == "duration" and self.ncol < 3:
            raise ValueError("weight='duration' needs a third (duration) column")
        fh, fw = (float(v) for v in frame_size)
        H, W = (int(v) for v in (output_shape if output_shape is not None else frame_size))
        if not (fh > 0 and fw > 0 and np.isfinite(fh) and np.isfinite(fw)) or H < 1 or W < 1:
            raise ValueError(f"frame_size {tuple(frame_size)} / output_shape {(H, W)}: positive sizes are required")
        K = self.K if K is None else K
        G = self.G if G is None else G
        dev = self._buf.device
        maps = torch.empty((G, H, W), dtype=torch.float64, device=dev)
        dropped = torch.empty(G, dtype=torch.int32, device=dev)
        if G:
            check(hip.lib().sp_fixation_maps(self.fix, self.ncol, self.start, self.count, self.group, K, G, H, W, fw, fh,
                                             WEIGHTS[weight], ptr(maps), ptr(dropped), hip.stream()), "sp_fixation_maps")
        return maps, dropped


def fixation_maps(scanpaths: Sequence, groups, frame_size, output_shape=None, weight: str = "binary", num_groups: Optional[int] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """scanpaths: list of [n, >= 2] arrays (x, y[, duration]) or structured fixation vectors (start_x, start_y, duration), of any
    length; groups[k]: the map of scanpath k; frame_size = (height, width) of the coordinate frame; output_shape (H, W) defaults to
    the frame; weight "binary" / "count" / "duration"; num_groups: the number of maps (default max(groups) + 1; a group without a
    scanpath gives a zero map).  Returns (maps [G,H,W] float64, dropped [G] int32: fixations outside the frame or non-finite), on the
    device.  Pixel: col = floor(x * W / frame_w), row = floor(y * H / frame_h); duration sums add in input order (np.add.at)."""
    return _Upload(scanpaths, groups, num_groups, _device()).rasterise(frame_size, output_shape, weight)


def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """scipy.ndimage's 1-D Gaussian kernel (_gaussian_kernel1d, order 0), [2 r + 1] with r = int(truncate * sigma + 0.5), bit for bit"""
    sd = float(sigma)
    radius = int(float(truncate) * sd + 0.5)
    if radius < 0:
        raise ValueError("negative radius")
    sigma2 = sd * sd
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def _half_kernel(sigma: float, truncate: float) -> np.ndarray:
    if sigma <= 1e-15:                    # scipy leaves such an axis unfiltered
        return np.ones(1)
    w = gaussian_weights(sigma, truncate)
    return np.ascontiguousarray(w[len(w) // 2:])


def density_maps(maps, sigma, truncate: float = 4.0, mode: str = "constant", normalise: Optional[str] = None) -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(map, sigma, mode=mode, cval=0, truncate=truncate) of every map of [G,H,W] (device or host; computed
    in float64), axis 0 first; sigma: a number or (sigma_y, sigma_x), 0 leaves that axis unfiltered; mode "constant", "reflect" or
    "nearest"; normalise None, "sum" or "max" divides each map by its sum / max (a zero map stays zero).  Returns a device tensor."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    if normalise not in NORMALISE:
        raise ValueError(f"normalise {normalise!r}: None, 'sum' or 'max'")
    sg = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if sg.size == 1:
        sg = np.repeat(sg, 2)
    if sg.size != 2 or not np.isfinite(sg).all() or (sg < 0).any():
        raise ValueError(f"sigma {sigma!r}: a non-negative number or (sigma_y, sigma_x)")
    if not (np.isfinite(truncate) and truncate >= 0):
        raise ValueError(f"truncate {truncate!r}")
    m = maps if isinstance(maps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(maps, dtype=np.float64)))
    if m.ndim != 3:
        raise ValueError(f"maps {tuple(m.shape)}: [G,H,W] is required")
    dev = _device()
    L = hip.lib()
    m = m.to(device=dev, dtype=torch.float64).contiguous()
    G, H, W = m.shape
    if max(H, W) > L.sp_gaussian_blur_maps_max_axis():
        raise ValueError(f"maps of {H}x{W}: the filter holds at most {L.sp_gaussian_blur_maps_max_axis()} pixels per axis")
    out = torch.empty_like(m)
    if G == 0:
        return out
    hy, hx = _half_kernel(sg[0], truncate), _half_kernel(sg[1], truncate)
    wts = torch.from_numpy(np.concatenate([hy, hx])).to(dev)
    ws = torch.empty(int(L.sp_gaussian_blur_maps_workspace(G, H, W)), dtype=torch.uint8, device=dev)      # the axis-0 result
    check(L.sp_gaussian_blur_maps(ptr(m), G, H, W, ptr(wts), len(hy) - 1, wts.data_ptr() + 8 * len(hy), len(hx) - 1, MODES[mode],
                                  NORMALISE[normalise], ptr(ws), ptr(out), hip.stream()), "sp_gaussian_blur_maps")
    return out


def _check_pred_maps(pred_maps, n_pred_scanpaths, G, shape) -> torch.Tensor:
    """the pred_maps of prediction='maps': a float64 [G, H, W] tensor (a host array becomes one), (H, W) the human maps' shape; what
    can be refused without a device is refused here (the values are checked where the maps are, next to the launches)"""
    if pred_maps is None:
        raise ValueError("prediction='maps' needs pred_maps [G, H, W]")
    if n_pred_scanpaths:
        raise ValueError("prediction='maps' takes no predicted scanpaths")
    m = pred_maps if isinstance(pred_maps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(pred_maps)))
    H, W = (int(v) for v in shape)
    if m.dtype != torch.float64 or tuple(m.shape) != (G, H, W):
        raise ValueError(f"pred_maps of dtype {m.dtype} and shape {tuple(m.shape)}: float64 [{G}, {H}, {W}], the shape of the human maps, "
                         "is required")
    return m.detach().contiguous()


def scanpath_saliency(gt_scanpaths: Sequence, gt_groups, pred_scanpaths: Sequence, pred_groups, frame_size, sigma, output_shape=None,
                      mode: str = "constant", pred_weight: str = "count", truncate: float = 4.0, num_groups: Optional[int] = None, *,
                      extra_metrics: Sequence[str] = (), image_groups=None, uniform_mix=None, baseline_sigma=None,
                      prediction: str = "scanpaths", pred_maps=None) -> Dict[str, torch.Tensor]:
    """How well the predicted scanpaths of each group predict where people looked.  Per group g (num_groups maps, default
    max(gt_groups) + 1): predicted density = the blur of the pred_weight map of all predicted scanpaths of g; then
      AUC_Judd = AUC_Judd(predicted density, binary human fixation map, jitter=False)   (Gaussian maps must not be jittered)
      NSS      = NSS(predicted density, binary human fixation map)
      KLdiv    = KLdiv(saliencyMap=predicted density, fixationMap=the same blur of the human count map)
    as float64 device tensors [G], with gt_dropped / pred_dropped int32 [G].  A group without human fixations or without
    predictions scores as the metric functions do on its empty map (NaN for AUC_Judd and NSS): nothing is left out.
    One upload of all fixations, 2 + 2 + 1 + 2 launches and one [G] copy of fixated-pixel counts, whatever G.

    extra_metrics: any of "sAUC", "CC", "SIM", "IG" (visual_attention_metrics.saliency_scores_pairs; the paper's formulae on
    sum-normalised maps, without the MATLAB benchmark code's min-max step) adds those keys and leaves the other ones bit for bit:
      image_groups [G]: the image group g was recorded on (default: every group is its own image);
      sAUC = the binary human map of g against the pool of pixels fixated in groups of OTHER images;
      CC, SIM = the predicted density against the human density KLdiv uses;
      IG = over the baseline Bm of g: the blur (baseline_sigma, default sigma) of the summed human count maps of all groups on other
           images, one blur per image; uniform_mix is then required (no default).
    prediction="centre_prior": the predicted density of g IS its Bm (pred_scanpaths must be empty): the floor a model has to beat.
    prediction="maps": pred_maps [G,H,W] (device or host, float64, finite and non-negative, the shape of the human maps -- e.g. the
    "maps" of expected_fixation_maps) takes the place of the rasterised prediction BEFORE the blur; pred_scanpaths must be empty,
    pred_weight is not read and pred_dropped is zeros.  Everything behind the rasterisation is the same code path.
    Extras cost one more upload of the human fixations and 2 + 2 + 1 + 1 launches, whatever G."""
    from . import visual_attention_metrics as M
    gt_groups = np.asarray(list(gt_groups), dtype=np.int64).reshape(-1)
    pred_groups = np.asarray(list(pred_groups), dtype=np.int64).reshape(-1)
    G = int(num_groups) if num_groups is not None else (int(gt_groups.max()) + 1 if gt_groups.size else 0)
    for name, grp in (("gt_groups", gt_groups), ("pred_groups", pred_groups)):
        if grp.size and (grp.min() < 0 or grp.max() >= G):
            raise ValueError(f"{name}: group index outside [0, {G})")
    extra = tuple(extra_metrics)
    unknown = [m for m in extra if m not in M.EXTRA_METRICS]
    if unknown or len(set(extra)) != len(extra):
        raise ValueError(f"extra_metrics {extra!r}: distinct names out of {M.EXTRA_METRICS}")
    if prediction not in ("scanpaths", "centre_prior", "maps"):
        raise ValueError(f"prediction {prediction!r}: 'scanpaths', 'centre_prior' or 'maps'")
    centre, given = prediction == "centre_prior", prediction == "maps"
    if centre and len(pred_scanpaths):
        raise ValueError("prediction='centre_prior' takes no predicted scanpaths")
    if pred_maps is not None and not given:
        raise ValueError(f"pred_maps is read with prediction='maps' only, not with prediction={prediction!r}")
    if given:
        pred_maps = _check_pred_maps(pred_maps, len(pred_scanpaths), G, output_shape if output_shape is not None else frame_size)
    alpha = M._check_mix(uniform_mix) if "IG" in extra else 0.0
    if image_groups is None:
        cls = np.arange(G, dtype=np.int64)
    else:
        cls = np.asarray(list(image_groups), dtype=np.int64).reshape(-1)
        if cls.shape[0] != G or (G and cls.min() < 0):
            raise ValueError(f"image_groups: one non-negative image index per group ({G}) is required, got {cls.shape[0]}")
    E = int(cls.max()) + 1 if G else 0
    dev = _device()
    if G == 0:
        z = torch.empty(0, dtype=torch.float64, device=dev)
        zi = torch.empty(0, dtype=torch.int32, device=dev)
        out = {"AUC_Judd": z, "NSS": z.clone(), "KLdiv": z.clone(), "gt_dropped": zi, "pred_dropped": zi.clone()}
        out.update({m: z.clone() for m in M.EXTRA_METRICS if m in extra})
        return out
    if pred_weight not in ("count", "duration", "binary"):
        raise ValueError(f"pred_weight {pred_weight!r}")
    # human scanpaths first, predicted ones shifted by G: one upload, maps [0, G) human and [G, 2G) predicted
    up = _Upload(list(gt_scanpaths) + list(pred_scanpaths), np.concatenate([gt_groups, pred_groups + G]), 2 * G, dev)
    if given:
        # the caller's maps stand where the rasterised prediction would: behind the human COUNT maps, in front of the blur
        gt_counts, gt_dropped = up.rasterise(frame_size, output_shape, "count", K=len(gt_groups), G=G)
        pm = pred_maps.to(dev)
        if not bool((torch.isfinite(pm) & (pm >= 0)).all()):
            raise ValueError("pred_maps: finite, non-negative values are required")
        counts, dropped = torch.cat([gt_counts, pm]), torch.cat([gt_dropped, torch.zeros_like(gt_dropped)])
    elif pred_weight == "count":
        counts, dropped = up.rasterise(frame_size, output_shape, "count")
    else:
        # the human density is always the blur of the COUNT map: rasterise the two halves with their own weights
        counts, dropped = up.rasterise(frame_size, output_shape, pred_weight)
        gt_counts, _ = up.rasterise(frame_size, output_shape, "count", K=len(gt_groups), G=G)
        counts[:G] = gt_counts
    binary, _ = up.rasterise(frame_size, output_shape, "binary", K=len(gt_groups), G=G)
    dens = density_maps(counts, sigma, truncate=truncate, mode=mode)
    P = dens.shape[1] * dens.shape[2]
    pred, human = dens[G:].reshape(G, P), dens[:G].reshape(G, P)
    base = None
    if centre or "IG" in extra:
        # per-image human count maps [0, E) and their total [E] from one more rasterisation; the counts are integers, so the
        # complement total - image is exact whatever the order.  One blur per image, then each group takes its image's map.
        ub = _Upload(list(gt_scanpaths) * 2, np.concatenate([cls[gt_groups], np.full(len(gt_groups), E, dtype=np.int64)]), E + 1, dev)
        per_image, _ = ub.rasterise(frame_size, output_shape, "count")
        others = per_image[E:] - per_image[:E]
        base = density_maps(others, sigma if baseline_sigma is None else baseline_sigma, truncate=truncate, mode=mode).reshape(E, P)
        if not np.array_equal(cls, np.arange(G)):
            base = base.index_select(0, torch.from_numpy(cls).to(dev))
    if centre:
        pred = base
    fixed = binary.reshape(G, P)
    nfix = M._count_positive(fixed)
    auc, nss, _ = M._saliency_metrics_device(pred, fixed, nfix=nfix)
    _, _, kld = M._saliency_metrics_device(pred, human, want_auc=False)
    out = {"AUC_Judd": auc, "NSS": nss, "KLdiv": kld, "gt_dropped": dropped[:G], "pred_dropped": dropped[G:]}
    if extra:
        cls_d = cnt = tot = None
        if "sAUC" in extra:
            cls_d, cnt, tot = M._pool_counts_device(fixed, cls, E)
        need_d = "CC" in extra or "SIM" in extra
        out.update(M._saliency_scores_device(pred, fixed if ("sAUC" in extra or "IG" in extra) else None, human if need_d else None,
                                             base if "IG" in extra else None, tot, 0, cnt, cls_d, E, alpha, nfix, want=extra))
    return out


# ---- the model's own fixation density, in closed form (csrc/scanexpect.hip in libscanpaths_amd_model.so) -----------------
_CELL_PIXELS = {}


def _model_library():
    """libscanpaths_amd_model.so, its limits held to this side's, or HipError"""
    L = hip.model_lib()
    if L.sp_model_max_fixations() != MAX_FIXATIONS or L.sp_model_max_cells() != MAX_CELLS:
        raise hip.HipError(f"kernel limits {L.sp_model_max_fixations()} / {L.sp_model_max_cells()}, this module expects "
                           f"{MAX_FIXATIONS} / {MAX_CELLS}")
    return L


def _check_sampler_frame(frame_size) -> Tuple[int, int]:
    """(height, width) of the sampler's frame: the sampler takes integers"""
    fh, fw = check_frame(frame_size)
    if int(fh) != fh or int(fw) != fw:
        raise ValueError(f"frame_size {tuple(frame_size)}: the sampler's frame has integer sizes")
    return int(fh), int(fw)


def _check_output_shape(output_shape, frame) -> Tuple[int, int]:
    if output_shape is None:
        return frame
    try:
        H, W = (int(v) for v in output_shape)
        exact = all(int(v) == v for v in output_shape)
    except (TypeError, ValueError):
        raise ValueError(f"output_shape {output_shape!r}: (H, W), two integers >= 1, is required") from None
    if not exact or H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"output_shape {tuple(output_shape)}: (H, W), two integers >= 1 with H * W within int32, is required")
    return H, W


def expected_cell_pixels(map_shape, frame_size, output_shape=None) -> np.ndarray:
    """int32 [Hm * Wm]: the output pixel row * W + col of every action-map cell -- BY DEFINITION the pixel in which the sampler's
    fixation of that cell lands: sp_generate_scanpath runs once on the P actions 1 .. P (its own float32 x and y for frame_size =
    (height, width), integers), and THE PIXEL RULE of fixation_maps, min(floor(v * n / frame), n - 1) in float64, is applied to what
    it emits.  One table, one rule: a sampled scanpath rasterised by fixation_maps and the closed form agree on every cell.  A cell
    whose fixation falls outside the frame raises.  output_shape (H, W) defaults to the frame.  Cached per (map_shape, frame_size,
    output_shape); the returned array is the cache's own and read-only."""
    Hm, Wm = check_map_shape(map_shape)
    fh, fw = _check_sampler_frame(frame_size)
    H, W = _check_output_shape(output_shape, (fh, fw))
    key = ((Hm, Wm), (fh, fw), (H, W))
    if key not in _CELL_PIXELS:
        dev, L, P = _device(), hip.lib(), Hm * Wm
        actions = torch.arange(1, P + 1, dtype=torch.int64, device=dev).reshape(P, 1)
        durations = torch.zeros((P, 1), dtype=torch.float32, device=dev)
        length, nfix = torch.empty(P, dtype=torch.float32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
        am, dm = torch.empty((P, 1), dtype=torch.float32, device=dev), torch.empty((P, 1), dtype=torch.float32, device=dev)
        fix = torch.empty((P, 1, 3), dtype=torch.float32, device=dev)
        check(L.sp_generate_scanpath(ptr(actions), ptr(durations), P, 1, Wm, Hm, fw, fh, ptr(length), ptr(am), ptr(dm), ptr(fix),
                                     ptr(nfix), hip.stream()), "sp_generate_scanpath")
        xy = fix.cpu().numpy().astype(np.float64).reshape(P, 3)
        x, y = xy[:, 0], xy[:, 1]
        if not (np.isfinite(xy).all() and (x >= 0).all() and (x < fw).all() and (y >= 0).all() and (y < fh).all()):
            raise ValueError(f"map_shape {(Hm, Wm)} on frame {(fh, fw)}: the sampler's fixation of a cell falls outside the frame")
        col = np.minimum(np.floor(x * W / fw), W - 1)
        row = np.minimum(np.floor(y * H / fh), H - 1)
        table = (row * W + col).astype(np.int32)
        table.setflags(write=False)
        _CELL_PIXELS[key] = table
    return _CELL_PIXELS[key]


def expected_durations(log_normal_mu, log_normal_sigma2) -> np.ndarray:
    """float64 [R, T]: the mean exp(mu + sigma2 * sigma2 / 2) of the duration the sampler draws at a step, exp(eps * sigma2 + mu) with
    eps standard normal (csrc/sampling.hip: sigma2 is the factor of eps) -- the step_weight of a duration-weighted
    expected_fixation_maps.  Computed on the host in float64 from the float32 values of the two [R, T] tensors."""
    def host(t, name):
        a = t.detach().to(torch.float32).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)
        if a.ndim != 2:
            raise ValueError(f"{name} of shape {a.shape}: [R, T] is required")
        return a.astype(np.float64)
    mu, s = host(log_normal_mu, "log_normal_mu"), host(log_normal_sigma2, "log_normal_sigma2")
    if mu.shape != s.shape:
        raise ValueError(f"log_normal_mu {mu.shape} and log_normal_sigma2 {s.shape}: one shape [R, T] is required")
    return np.exp(mu + s * s / 2.0)


def expected_fixation_maps(probs, row_groups, n_groups, *, min_length, max_steps, frame_size, output_shape=None, map_shape=None,
                           step_weight=None) -> Dict[str, object]:
    """The expected "count" (or weighted) fixation map of the sampler's scanpaths, exactly and without sampling: what
    fixation_maps(samples, ..., "count") / number of samples converges to.  probs: device tensor [R, T, 1 + P] of the model's
    eval-mode step distributions (any float dtype; detached and read as float32); row_groups [R] in [0, n_groups): the map each row
    is added into, in ascending row index; min_length: the sampler's; max_steps <= 64: only the first max_steps steps count;
    frame_size = (height, width), the sampler's integers (all three required); output_shape (H, W) defaults to the frame; map_shape
    = (Hm, Wm) defaults to (30, 40) for 1201 actions only, at most 2048 cells; step_weight: None or [R, T] finite and non-negative,
    the weight of a fixation of step t -- expected_durations(mu, sigma2) gives the "duration" map.
    With Z, D, q, c, A of saccade_expectation (bad rows agree): e_r(i) = sum_t c_t(i) (A_t s_t), w_t = A_t (1 - q_t), a cell's mass
    goes to the pixel of expected_cell_pixels (the order of every sum: csrc/scanexpect.hip).
    Returns {"maps": float64 [n_groups, H, W] ON THE DEVICE (ready for scanpath_saliency(prediction="maps")), "fixations": float64 [R]
    numpy = the expected number of fixations sum_t w_t, "bad": int32 [R] numpy: 1 for a row with a step without mass (fixations NaN,
    nothing added)}.  R = 0: zero maps, and no device is asked for.  There is no CPU path."""
    min_length, max_steps = check_min_length(min_length), check_steps(max_steps)
    if max_steps > MAX_FIXATIONS:
        raise ValueError(f"max_steps {max_steps}: at most {MAX_FIXATIONS} steps count")
    frame = _check_sampler_frame(frame_size)
    H, W = _check_output_shape(output_shape, frame)
    if not isinstance(probs, torch.Tensor) or probs.dim() != 3 or probs.shape[1] < 1 or probs.shape[2] < 2:
        raise ValueError("probs: an [R, T, A] tensor with T >= 1 and A >= 2 is required")
    R, T, A = (int(v) for v in probs.shape)
    shape = check_map(A, map_shape, max_cells=MAX_CELLS)
    grp, G = check_groups(row_groups, R, n_groups, "row")
    sw = None
    if step_weight is not None:
        sw = step_weight.detach().cpu().numpy() if isinstance(step_weight, torch.Tensor) else np.asarray(step_weight)
        sw = np.ascontiguousarray(sw, dtype=np.float64)
        if sw.shape != (R, T) or not np.isfinite(sw).all() or (sw < 0).any():
            raise ValueError(f"step_weight of shape {sw.shape}: finite, non-negative values [{R}, {T}] are required")
    if R == 0:
        return {"maps": torch.zeros((G, H, W), dtype=torch.float64), "fixations": np.zeros(0, np.float64), "bad": np.zeros(0, np.int32)}
    cell_pixel = expected_cell_pixels(shape, frame, (H, W))
    dev, L = _device(), _model_library()
    sections = dict(row_group=grp, cell_pixel=cell_pixel)
    if sw is not None:
        sections["step_weight"] = sw
    buf, at = _batch.upload(sections, dev)
    p = probs.detach().to(device=dev, dtype=torch.float32).contiguous()
    work = torch.empty(int(L.sp_model_fixation_expectation_workspace(R, T, *shape, G, max_steps)), dtype=torch.float64, device=dev)
    maps = torch.empty((G, H, W), dtype=torch.float64, device=dev)
    out = _batch.Out({"fixations": (np.float64, R), "bad": (np.int32, R)}, dev)
    check(L.sp_model_fixation_expectation(ptr(p), at.get("step_weight"), at["row_group"], R, T, *shape, G, min_length, max_steps,
                                          at["cell_pixel"], H, W, ptr(work), ptr(maps), out.ptr("fixations"), out.ptr("bad"),
                                          hip.stream()), "sp_model_fixation_expectation")
    return dict(out.host(), maps=maps)
