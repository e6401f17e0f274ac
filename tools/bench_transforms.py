"""Time the dataset transforms of one batch on the device beside the host path they replace.

Device: ``resize_normalise_images`` of bs images (480x640 RGB uint8 -> 320x512) and ``attention_maps`` of bs AiR box maps (480x640
float32 -> 30x40, / max).  Reported: the kernel time alone (HIP events around the launches on inputs already on the device) and the
whole call (host packing, upload, launches, synchronise).  Host: Pillow BILINEAR + numpy ToTensor / Normalize, and
scipy.ndimage.gaussian_filter + the bilinear step for one map, per sample (skipped where Pillow / scipy do not import).

    python tools/bench_transforms.py [--bs 32] [--iters 50] [--out profiles/bench_transforms.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _wall_ms(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from scanpaths_amd import hip, transforms as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_transforms needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(7))
    imgs = [rng.integers(0, 256, size=(480, 640, 3), dtype=np.uint8) for _ in range(a.bs)]
    maps = []
    for _ in range(a.bs):
        m = np.zeros((480, 640), np.float32)
        for _ in range(3):
            y, x = int(rng.integers(0, 400)), int(rng.integers(0, 560))
            m[y:y + int(rng.integers(20, 200)), x:x + int(rng.integers(20, 300))] = 1
        maps.append(m)
    H, W = 320, 512
    res = {"bs": a.bs, "images": "480x640 -> 320x512", "maps": "480x640 -> 30x40"}

    # kernel only: inputs already on the device
    src, off_d, meta_d = T._pack_images(imgs, H, W, dev)
    out = torch.empty((a.bs, 3, H, W), dtype=torch.float32, device=dev)
    m32, s32 = [float(np.float32(v)) for v in T.IMAGENET_MEAN], [float(np.float32(v)) for v in T.IMAGENET_STD]

    def img_kernel():
        hip.check(hip.lib().sp_resize_normalize_images(hip.ptr(src), hip.ptr(off_d), hip.ptr(meta_d), a.bs, H, W, *m32, *s32,
                                                        hip.ptr(out), hip.stream()), "sp_resize_normalize_images")
    msrc = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).to(dev)
    moff = np.arange(a.bs, dtype=np.int64) * 480 * 640
    mdims = np.tile(np.array([[480, 640]], np.int64), (a.bs, 1))

    def map_call_on_device():
        T._resize_packed(msrc, False, moff, mdims, 1, (30, 40), 1, 0.0, torch.float32, dev, False)
    for fn in (img_kernel, map_call_on_device):
        fn()
    torch.cuda.synchronize()
    res["image_kernel_ms"] = _events_ms(img_kernel, a.iters)
    res["image_bytes_moved_MB"] = (src.numel() + out.numel() * 4) / 1e6
    res["image_kernel_GBps"] = res["image_bytes_moved_MB"] / res["image_kernel_ms"]
    res["map_device_ms"] = _events_ms(map_call_on_device, a.iters)      # includes the small table uploads
    # whole calls from host arrays
    res["image_call_ms"] = _wall_ms(lambda: T.resize_normalise_images(imgs, (H, W), device=dev), max(5, a.iters // 5))
    res["map_call_ms"] = _wall_ms(lambda: T.attention_maps(maps, (30, 40), device=dev), max(5, a.iters // 5))

    # host path, per sample
    try:
        from PIL import Image
        mean = np.array(T.IMAGENET_MEAN, np.float32)[:, None, None]
        std = np.array(T.IMAGENET_STD, np.float32)[:, None, None]

        def host_img(im):
            r = np.asarray(Image.fromarray(im).resize((W, H), Image.BILINEAR))
            return (r.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - mean) / std
        n = min(a.bs, 8)
        t = time.perf_counter()
        for im in imgs[:n]:
            host_img(im)
        res["host_image_ms_per_sample"] = (time.perf_counter() - t) * 1e3 / n
    except ImportError:
        res["host_image_ms_per_sample"] = None
    try:
        spec = importlib.util.spec_from_file_location("g", os.path.join(ROOT, "tests", "golden", "make_golden_transforms.py"))
        g = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(g)
        n = min(a.bs, 4)
        t = time.perf_counter()
        for m in maps[:n]:
            r = g.skimage_resize(m, (30, 40))
            r /= r.max()
        res["host_map_ms_per_sample"] = (time.perf_counter() - t) * 1e3 / n
    except ImportError:
        res["host_map_ms_per_sample"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
