"""The reference's per-sample image and attention-map transforms, batched on the device (csrc/transforms.hip).

* ``resize_normalise_images``: ``transforms.Compose([Resize((H, W)), ToTensor(), Normalize(mean, std)])`` of torchvision 0.7 on
  PIL RGB images (AiR/train.py:43-46, OSIE/train.py:41-45, COCO_Search18/train.py:41-45), stacked: bit-identical to Pillow's 8-bit
  BILINEAR resize followed by torch's float32 ``div(255)``, ``sub_(mean)``, ``div_(std)``.
* ``resize_maps``: skimage 0.17.2 ``resize(map, output_shape)`` with its defaults (anti-aliasing on, mode 'reflect', order 1, clip),
  optionally followed by the datasets' normalisation; ``attention_maps`` is AiR's (AiR/dataset/dataset.py:151-154: ``/= max``) and
  COCO-Search18's (COCO_Search18/dataset/dataset.py:159: ``/= max + 1e-7``) attention map.
* ``attention_maps_from_detections`` / ``scene_graph_maps``: the binary box maps are rasterised on the device from integer boxes
  (COCO_Search18/dataset/dataset.py:150-160; AiR ``get_scene_graph_info``, AiR/dataset/dataset.py:63-97) and resized there.

The host only validates, packs the ragged inputs into one buffer and builds the coefficient tables (Pillow's fixed-point bilinear
weights, scipy's Gaussian weights, both in float64 and cached per size pair).  There is no CPU path: without a HIP device the calls
raise ``HipError`` after validating their arguments.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .hip import check, ptr

IMAGENET_MEAN = (0.485, 0.456, 0.406)           # the reference's Normalize arguments (AiR/train.py:45)
IMAGENET_STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22                              # Pillow's fixed-point precision for 8-bit images
MAX_OBJECTS = 5                                  # get_scene_graph_info's max_object_num (AiR/dataset/dataset.py:64)


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise hip.HipError("scanpaths_amd.transforms runs on a HIP device only (no CPU path)")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.HipError("scanpaths_amd.transforms runs on a HIP device only (no CPU path)")
    return device


def _size2(size, what) -> Tuple[int, int]:
    if isinstance(size, int):
        raise ValueError(f"{what}: give (height, width); an int keeps the aspect ratio in torchvision and is not supported")
    h, w = (int(s) for s in size)
    if h < 1 or w < 1:
        raise ValueError(f"{what}: sizes must be >= 1, got {size}")
    return h, w


# ---------------------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=256)
def pil_bilinear_coeffs(in_size: int, out_size: int) -> Tuple[int, np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BILINEAR (support 1) over one axis: (ksize, bounds [out][2] = (min, n),
    coefficients [out][ksize] int32 with PRECISION_BITS fractional bits).  Python floats are IEEE doubles, as in Pillow's C."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = []
        ww = 0.0
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - t if t < 1.0 else 0.0
            k.append(w)
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = [int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)) for w in k]
    return ksize, bounds, kk


def _table_words(in_size: int, out_size: int) -> np.ndarray:
    ksize, bounds, kk = pil_bilinear_coeffs(in_size, out_size)
    return np.concatenate([np.array([ksize], np.int32), bounds.reshape(-1), kk.reshape(-1)])


def _as_hwc_uint8(img, i: int):
    """numpy / torch uint8 [H, W, 3], or a PIL image (converted to RGB as the reference's loader does)"""
    if hasattr(img, "convert") and hasattr(img, "size") and not isinstance(img, (np.ndarray, torch.Tensor)):
        img = np.asarray(img.convert("RGB"))
    if isinstance(img, torch.Tensor):
        if img.dtype != torch.uint8:
            raise TypeError(f"image {i}: dtype {img.dtype}, expected torch.uint8 (decoded 8-bit RGB, HWC)")
    else:
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise TypeError(f"image {i}: dtype {img.dtype}, expected uint8 (decoded 8-bit RGB, HWC)")
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image {i}: shape {tuple(img.shape)}, expected [H, W, 3] (RGB, channels last)")
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image {i}: empty image {tuple(img.shape)}")
    return img


def _pack_images(imgs, H: int, W: int, dev):
    """(packed uint8 pixels, byte offsets, int32 meta + Pillow tables) on the device for sp_resize_normalize_images"""
    B = len(imgs)
    # meta [B][4] = (H_b, W_b, horizontal table, vertical table), then one table per distinct (in, out) pair
    meta = np.zeros(4 * B, np.int32)
    tables, words = {}, 4 * B
    parts = []
    for b, im in enumerate(imgs):
        hi, wi = int(im.shape[0]), int(im.shape[1])
        offs = []
        for key in ((wi, W), (hi, H)):
            if key not in tables:
                t = _table_words(*key)
                tables[key] = words
                parts.append(t)
                words += t.size
            offs.append(tables[key])
        meta[4 * b: 4 * b + 4] = (hi, wi, offs[0], offs[1])
    meta_d = torch.from_numpy(np.concatenate([meta] + parts)).to(dev)
    sizes = np.array([im.shape[0] * im.shape[1] * 3 for im in imgs], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    if all(isinstance(im, torch.Tensor) and im.device == dev for im in imgs):
        src = torch.cat([im.reshape(-1) for im in imgs])
    else:
        src = torch.from_numpy(np.concatenate([np.ascontiguousarray(im if isinstance(im, np.ndarray) else im.cpu().numpy()).reshape(-1)
                                               for im in imgs])).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    return src, off_d, meta_d


def resize_normalise_images(images: Sequence, size=(320, 512), mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None) -> torch.Tensor:
    """``torch.stack([Compose([Resize(size), ToTensor(), Normalize(mean, std)])(img) for img in images])`` -> float32 [B, 3, H, W]
    on the device, bit-identical to Pillow BILINEAR + torchvision 0.7's float32 arithmetic.  images: uint8 RGB HWC numpy arrays or
    torch tensors (any sizes), or PIL images."""
    imgs = [_as_hwc_uint8(im, i) for i, im in enumerate(images)]
    if not imgs:
        raise ValueError("empty batch")
    H, W = _size2(size, "size")
    mean32 = [float(np.float32(m)) for m in mean]
    std32 = [float(np.float32(s)) for s in std]
    if len(mean32) != 3 or len(std32) != 3:
        raise ValueError("mean and std need 3 values (RGB)")
    B = len(imgs)
    if B > 65535:
        raise ValueError("at most 65535 images per call")
    dev = _device(device)

    src, off_d, meta_d = _pack_images(imgs, H, W, dev)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    check(hip.lib().sp_resize_normalize_images(ptr(src), ptr(off_d), ptr(meta_d), B, H, W, *mean32, *std32, ptr(out), hip.stream()),
          "sp_resize_normalize_images")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------------------------------------------------------------
def antialias_sigma(in_size: int, out_size: int) -> float:
    """skimage 0.17.2 resize: anti_aliasing_sigma = max(0, (in / out - 1) / 2) per axis"""
    return max(0.0, (float(in_size) / float(out_size) - 1.0) / 2.0)


@functools.lru_cache(maxsize=256)
def gaussian_half_kernel(sigma: float) -> np.ndarray:
    """scipy.ndimage.gaussian_filter1d's weights (truncate 4.0) at distances 0..radius; [1.0] where ndimage skips the axis
    (sigma <= 1e-15)"""
    if sigma <= 1e-15:
        return np.ones(1, np.float64)
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def _as_map(m, i: int):
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    m = np.asarray(m)
    if m.dtype not in (np.float32, np.uint8):
        raise TypeError(f"map {i}: dtype {m.dtype}, expected float32 or uint8 (uint8 values are read as their float32 values)")
    if m.ndim not in (2, 3):
        raise ValueError(f"map {i}: shape {m.shape}, expected [h, w] or [h, w, C]")
    if min(m.shape) < 1:
        raise ValueError(f"map {i}: empty map {m.shape}")
    return m


_NORM = {None: 0, "max": 1, "max_eps": 2}


def _resize_packed(src_d, u8: bool, off: np.ndarray, dims: np.ndarray, C: int, output_shape, norm: int, eps: float, dtype, dev,
                   channel_axis: bool) -> torch.Tensor:
    h, w = output_shape
    B = dims.shape[0]
    filt = np.zeros((B, 4), np.int32)
    kernels, chunks, n = {}, [], 0
    for b in range(B):
        for a, (i, o) in enumerate(((int(dims[b, 0]), h), (int(dims[b, 1]), w))):
            s = antialias_sigma(i, o)
            if s not in kernels:
                kw = gaussian_half_kernel(s)
                kernels[s] = n
                chunks.append(kw)
                n += kw.size
            filt[b, 2 * a:2 * a + 2] = (gaussian_half_kernel(s).size - 1, kernels[s])
    ints = torch.from_numpy(np.concatenate([dims.reshape(-1).astype(np.int32), filt.reshape(-1)])).to(dev)
    wts = torch.from_numpy(np.concatenate(chunks)).to(dev)
    off_d = torch.from_numpy(off.astype(np.int64)).to(dev)
    f64 = dtype == torch.float64
    out = torch.empty((B, h, w, C) if channel_axis else (B, h, w), dtype=torch.float64 if f64 else torch.float32, device=dev)
    wmax = int(dims[:, 1].max())
    if B * 2 * h * wmax * C >= 2 ** 31 or int(dims[:, 1].max()) * int(dims[:, 0].max()) * C >= 2 ** 31:
        raise ValueError("maps too large for one call")
    ws = hip.workspace(int(hip.lib().sp_resize_maps_workspace(B, h, w, C, wmax)), dev)
    check(hip.lib().sp_resize_maps(ptr(src_d), int(u8), ptr(off_d), ptr(ints), ptr(ints[2 * B:]), ptr(wts), B, C, h, w, wmax, norm,
                                   float(eps), int(f64), ptr(ws), ptr(out), hip.stream()), "sp_resize_maps")
    return out


def resize_maps(maps: Sequence, output_shape=(30, 40), normalise=None, eps: float = 0.0, dtype=torch.float32, device=None) -> torch.Tensor:
    """skimage 0.17.2 ``resize(m, output_shape)`` (defaults: anti-aliasing, order 1, mode 'reflect', clip) of every map, stacked ->
    [B, h, w] or [B, h, w, C] on the device.  maps: float32 or uint8 (read as ``.astype(np.float32)``) arrays [h_i, w_i] or
    [h_i, w_i, C] of any sizes (one C per batch).  normalise: None, "max" (``/= max``) or "max_eps" (``/= max + eps``), in float64;
    dtype float32 rounds the float64 result once, float64 keeps it (what ``torch.from_numpy`` of the reference's arrays holds)."""
    if normalise not in _NORM:
        raise ValueError(f"normalise must be one of {list(_NORM)}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64")
    ms = [_as_map(m, i) for i, m in enumerate(maps)]
    if not ms:
        raise ValueError("empty batch")
    if len({m.ndim for m in ms}) != 1 or len({m.shape[2] for m in ms if m.ndim == 3}) > 1:
        raise ValueError("all maps of a batch need the same number of channels")
    u8 = ms[0].dtype == np.uint8
    if any((m.dtype == np.uint8) != u8 for m in ms):
        raise TypeError("all maps of a batch need the same dtype")
    h, w = _size2(output_shape, "output_shape")
    if len(ms) > 65535:
        raise ValueError("at most 65535 maps per call")
    dev = _device(device)
    C = ms[0].shape[2] if ms[0].ndim == 3 else 1
    dims = np.array([m.shape[:2] for m in ms], np.int64)
    sizes = np.array([m.size for m in ms], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    src = torch.from_numpy(np.concatenate([np.ascontiguousarray(m).reshape(-1) for m in ms])).to(dev)
    return _resize_packed(src, u8, off, dims, C, (h, w), _NORM[normalise], eps, dtype, dev, ms[0].ndim == 3)


def attention_maps(box_maps: Sequence, action_map=(30, 40), eps: float = 0.0, dtype=torch.float32, device=None) -> torch.Tensor:
    """The attention_map of AiR.__getitem__ (eps = 0: ``resize`` then ``/= max``, AiR/dataset/dataset.py:151-154; an all-zero map
    gives NaN as there) or COCO_Search18.__getitem__ (eps = 1e-7: ``/= max + 1e-7``, COCO_Search18/dataset/dataset.py:159-160),
    stacked as collate_func does: [B, 1, h, w]"""
    if any(np.ndim(m) != 2 for m in box_maps):
        raise ValueError("attention box maps are 2-D [h, w]")
    return resize_maps(box_maps, action_map, "max_eps" if eps else "max", eps, dtype, device).unsqueeze(1)


def _clip_slice(a: int, b: int, n: int) -> Tuple[int, int]:
    """numpy basic-slicing bounds of m[a:b] along an axis of length n (negative indices count from the end)"""
    lo, hi, _ = slice(a, b).indices(n)
    return lo, max(lo, hi)


def _rasterize(boxes_per_sample: List[List[Tuple[int, int, int, int, int]]], dims: np.ndarray, C: int, dev):
    """uint8 box maps [h_b, w_b, C], packed, rasterised on the device; boxes (y0, y1, x0, x1, channel) already clipped"""
    B = dims.shape[0]
    cnt = np.array([len(bx) for bx in boxes_per_sample], np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    flat = [v for bx in boxes_per_sample for box in bx for v in box]
    sizes = dims[:, 0] * dims[:, 1] * C
    if int(sizes.max()) >= 2 ** 31:
        raise ValueError("a box map has more than 2^31 - 1 elements")
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    ints = torch.from_numpy(np.concatenate([dims.reshape(-1).astype(np.int32), start, np.array(flat, np.int32)])).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    dst = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=dev)
    boxes_d = ints[3 * B + 1:] if flat else None
    check(hip.lib().sp_rasterize_boxes(ptr(boxes_d), ptr(ints[2 * B:]), ptr(off_d), ptr(ints), B, C, int(sizes.max()), ptr(dst),
                                       hip.stream()), "sp_rasterize_boxes")
    return dst, off


def attention_maps_from_detections(dets_per_sample: Sequence[Sequence[dict]], task_per_sample: Sequence[str], det_sizes,
                                   action_map=(30, 40), eps: float = 1e-7, dtype=torch.float32, device=None) -> torch.Tensor:
    """COCO_Search18.__getitem__'s attention map (COCO_Search18/dataset/dataset.py:150-160) for a batch: the boxes of the searched
    category (``int(bbox[k])``, (x_min, y_min, x_max, y_max)) are drawn into a [det_h, det_w] map on the device, resized like skimage
    and divided by max + eps -> [B, 1, h, w].  det_sizes: one (det_h, det_w) per sample, or one pair for all."""
    B = len(dets_per_sample)
    if B == 0:
        raise ValueError("empty batch")
    if len(task_per_sample) != B:
        raise ValueError("one task per sample")
    sizes = np.asarray(det_sizes, dtype=np.int64).reshape(-1, 2)
    if sizes.shape[0] == 1:
        sizes = np.repeat(sizes, B, axis=0)
    if sizes.shape[0] != B or (sizes < 1).any():
        raise ValueError("det_sizes: one positive (height, width) per sample")
    h, w = _size2(action_map, "action_map")
    boxes = []
    for b in range(B):
        bx = []
        for det in dets_per_sample[b]:
            if det["category"] == task_per_sample[b]:
                x_min, y_min, x_max, y_max = (int(det["bbox"][k]) for k in range(4))
                y0, y1 = _clip_slice(y_min, y_max, int(sizes[b, 0]))
                x0, x1 = _clip_slice(x_min, x_max, int(sizes[b, 1]))
                bx.append((y0, y1, x0, x1, 0))
        boxes.append(bx)
    dev = _device(device)
    dst, off = _rasterize(boxes, sizes, 1, dev)
    out = _resize_packed(dst, True, off, sizes, 1, (h, w), 2 if eps else 1, eps, dtype, dev, False)
    return out.unsqueeze(1)


def scene_graph_maps(fixation_records: Sequence[dict], resize=(240, 320), dtype=torch.float32, device=None) -> Dict[str, torch.Tensor]:
    """AiR's get_scene_graph_info (AiR/dataset/dataset.py:63-97) for a batch: the question / full-answer objects ((x, y, h, w) of
    ``record["objects"][name]``, at most 5 each) drawn as channels of [height, width, 5] maps on the device, resized to ``resize``
    with skimage's defaults -> question_objects_pos / fullAnswer_objects_pos [B, h, w, 5] and the two masks [B, 5]."""
    B = len(fixation_records)
    if B == 0:
        raise ValueError("empty batch")
    h, w = _size2(resize, "resize")
    dims = np.array([(int(f["height"]), int(f["width"])) for f in fixation_records], np.int64)
    if (dims < 1).any():
        raise ValueError("height and width must be >= 1")
    out = {}
    for key in ("question", "fullAnswer"):
        masks = np.zeros((B, MAX_OBJECTS), np.float32)
        boxes = []
        for b, f in enumerate(fixation_records):
            objs = [f["objects"][name] for name in f["annotations"][key].values()]
            if len(objs) > MAX_OBJECTS:
                raise ValueError(f"record {b}: {len(objs)} {key} objects, the reference's maps hold {MAX_OBJECTS}")
            bx = []
            for idx, o in enumerate(objs):
                x, y, oh, ow = int(o["x"]), int(o["y"]), int(o["h"]), int(o["w"])
                y0, y1 = _clip_slice(y, y + oh, int(dims[b, 0]))
                x0, x1 = _clip_slice(x, x + ow, int(dims[b, 1]))
                bx.append((y0, y1, x0, x1, idx))
                masks[b, idx] = 1
            boxes.append(bx)
        dev = _device(device)
        dst, off = _rasterize(boxes, dims, MAX_OBJECTS, dev)
        out[f"{key}_objects_pos"] = _resize_packed(dst, True, off, dims, MAX_OBJECTS, (h, w), 0, 0.0, dtype, dev, True)
        out[f"{key}_objects_masks"] = torch.from_numpy(masks).to(dev)
    return out
