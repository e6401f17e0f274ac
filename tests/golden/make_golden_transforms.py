"""Goldens of scanpaths_amd.transforms (tests/golden/transforms.npz).

Images: Pillow's ``Image.resize((W, H), Image.BILINEAR)`` of seeded random RGB images, then torchvision 0.7's ToTensor / Normalize
arithmetic in torch-CPU float32 (``img.float().div(255)``, ``sub_(mean)``, ``div_(std)``).  Small batches are stored as arrays; the
full-size ones (480x640, 600x800, 1050x1680 -> 320x512 and 240x320) as their PCG64 seed and the SHA-256 of the expected float32
[B, 3, H, W] tensor (the bar is bit-exact).

Maps: skimage 0.17.2 ``resize(m, out)`` with its defaults, restated: ``scipy.ndimage.gaussian_filter`` (the call skimage makes:
sigma = max(0, (in/out - 1)/2) per spatial axis, mode 'mirror', truncate 4) and a numpy restatement of its metric-warp bilinear
step ('reflect' borders) and clip.  scikit-image is not installed here, so that step is not pinned against the library itself.
Stored: seeds, shapes and the expected float64 maps before the datasets' normalisation.

The input generators below use numpy only; the GPU tests import them to rebuild the same inputs.

    python tests/golden/make_golden_transforms.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# (name, seed, source sizes, output size)
IMAGE_SMALL = [
    ("mixed", 11, [(40, 50), (5, 7), (30, 9), (13, 17), (1, 1), (23, 31), (9, 40), (101, 3)], (13, 17)),
    ("row", 12, [(4, 3), (1, 9), (6, 20), (1, 1)], (1, 9)),
]
IMAGE_FULL = [
    ("to320x512", 21, [(480, 640), (600, 800), (1050, 1680)], (320, 512)),
    ("to240x320", 22, [(480, 640), (600, 800), (1050, 1680)], (240, 320)),
]
# (name, seed, source shapes [h, w] or [h, w, C], output size, uint8 binary box maps?)
MAPS = [
    ("2d", 31, [(480, 640), (75, 100), (98, 131), (30, 40), (12, 16), (1, 80)], (30, 40), False),
    ("2d_u8", 32, [(105, 105), (512, 512), (20, 13), (32, 32), (1, 32)], (32, 32), True),
    ("5ch", 33, [(60, 80, 5), (384, 512, 5), (24, 32, 5), (79, 105, 5)], (24, 32), True),
    ("5ch_f32", 34, [(60, 80, 5), (10, 12, 5)], (24, 32), False),
]


def make_images(seed, sizes):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def make_maps(seed, shapes, u8):
    """float32 noise maps, or uint8 binary maps of up to 4 random boxes per channel"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for shp in shapes:
        if not u8:
            out.append(rng.random(shp, dtype=np.float32))
            continue
        m = np.zeros(shp, np.uint8)
        C = shp[2] if len(shp) == 3 else 1
        for c in range(C):
            for _ in range(int(rng.integers(1, 5))):
                y0, x0 = int(rng.integers(0, shp[0])), int(rng.integers(0, shp[1]))
                y1, x1 = y0 + int(rng.integers(1, shp[0] + 1)), x0 + int(rng.integers(1, shp[1] + 1))
                if len(shp) == 3:
                    m[y0:y1, x0:x1, c] = 1
                else:
                    m[y0:y1, x0:x1] = 1
        out.append(m)
    return out


def torchvision_images(imgs, size):
    """Compose([Resize(size), ToTensor(), Normalize(MEAN, STD)]) of torchvision 0.7 on PIL images, stacked"""
    import torch
    from PIL import Image
    mean = torch.as_tensor(MEAN, dtype=torch.float32)[:, None, None]
    std = torch.as_tensor(STD, dtype=torch.float32)[:, None, None]
    out = []
    for im in imgs:
        r = np.asarray(Image.fromarray(im).resize((size[1], size[0]), Image.BILINEAR))
        t = torch.from_numpy(r.copy()).permute(2, 0, 1).contiguous().float().div(255)
        out.append(t.sub_(mean).div_(std))
    return torch.stack(out).numpy()


def _reflect(i, n):
    """skimage's 'reflect' coordinate map (ndimage 'mirror': the edge pixel is not repeated)"""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def skimage_resize(m, out):
    """skimage 0.17.2 resize(m.astype(np.float32), out): anti-aliasing Gaussian, bilinear metric warp, mode 'reflect', clip"""
    from scipy import ndimage
    x = m.astype(np.float32)
    sig = [max(0.0, (x.shape[a] / out[a] - 1.0) / 2.0) for a in range(2)] + [0.0] * (x.ndim - 2)
    f = ndimage.gaussian_filter(x, sig, mode="mirror", truncate=4.0)
    hi, wi = f.shape[:2]
    r = (hi / out[0]) * (np.arange(out[0], dtype=np.float64) + 0.5) - 0.5
    c = (wi / out[1]) * (np.arange(out[1], dtype=np.float64) + 0.5) - 0.5
    r0, r1, c0, c1 = np.floor(r), np.ceil(r), np.floor(c), np.ceil(c)
    dr, dc = (r - r0)[:, None], (c - c0)[None, :]
    if f.ndim == 3:
        dr, dc = dr[..., None], dc[..., None]
    R0, R1 = _reflect(r0.astype(np.int64), hi), _reflect(r1.astype(np.int64), hi)
    C0, C1 = _reflect(c0.astype(np.int64), wi), _reflect(c1.astype(np.int64), wi)
    g = f.astype(np.float64)
    tl, tr, bl, br = g[R0][:, C0], g[R0][:, C1], g[R1][:, C0], g[R1][:, C1]
    v = (1 - dr) * ((1 - dc) * tl + dc * tr) + dr * ((1 - dc) * bl + dc * br)
    return np.clip(v, f.min(), f.max())


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests.helpers import save_npz
    d = {"mean": np.array(MEAN, np.float64), "std": np.array(STD, np.float64)}
    for name, seed, sizes, out in IMAGE_SMALL:
        d[f"img_{name}_expected"] = torchvision_images(make_images(seed, sizes), out)
    for name, seed, sizes, out in IMAGE_FULL:
        e = np.ascontiguousarray(torchvision_images(make_images(seed, sizes), out), dtype=np.float32)
        d[f"img_{name}_sha256"] = np.frombuffer(hashlib.sha256(e.tobytes()).digest(), np.uint8).copy()
    for name, seed, shapes, out, u8 in MAPS:
        d[f"map_{name}_expected"] = np.stack([skimage_resize(m, out) for m in make_maps(seed, shapes, u8)])
    save_npz(os.path.join(HERE, "transforms.npz"), d)
    for k, v in d.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
