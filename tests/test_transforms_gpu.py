"""GPU: scanpaths_amd.transforms against tests/golden/transforms.npz (make_golden_transforms.py).  Images are bit-identical to Pillow
BILINEAR + torchvision 0.7's float32 ToTensor / Normalize; maps are within 1e-6 * max|ref| of the skimage 0.17.2 resize restatement;
the device-rasterised box maps equal the host-drawn ones; collate_raw builds the reference collate_func's batch."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_npz

pytestmark = pytest.mark.gpu


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_transforms", os.path.join(GOLDEN, "make_golden_transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


@pytest.fixture(scope="module")
def golden():
    return load_npz(os.path.join(GOLDEN, "transforms.npz"))


@pytest.mark.parametrize("case", G.IMAGE_SMALL, ids=[c[0] for c in G.IMAGE_SMALL])
def test_ragged_image_batch_is_bit_identical(golden, case):
    from scanpaths_amd.transforms import resize_normalise_images
    name, seed, sizes, out = case
    imgs = G.make_images(seed, sizes)
    got = resize_normalise_images(imgs, out)
    exp = torch.from_numpy(golden[f"img_{name}_expected"]).cuda()
    assert got.shape == exp.shape and got.dtype == torch.float32
    assert torch.equal(got, exp), (got - exp).abs().max().item()
    # torch uint8 input on the device, and host tensors, give the same
    assert torch.equal(resize_normalise_images([torch.from_numpy(im).cuda() for im in imgs], out), exp)
    assert torch.equal(resize_normalise_images([torch.from_numpy(im) for im in imgs], out), exp)


@pytest.mark.parametrize("case", G.IMAGE_FULL, ids=[c[0] for c in G.IMAGE_FULL])
def test_full_size_images_hash_equal(golden, case):
    from scanpaths_amd.transforms import resize_normalise_images
    name, seed, sizes, out = case
    got = resize_normalise_images(G.make_images(seed, sizes), out).cpu().contiguous().numpy()
    assert hashlib.sha256(got.tobytes()).digest() == golden[f"img_{name}_sha256"].tobytes()


@pytest.mark.parametrize("case", G.MAPS, ids=[c[0] for c in G.MAPS])
def test_map_resize_matches_the_skimage_restatement(golden, case):
    from scanpaths_amd.transforms import resize_maps
    name, seed, shapes, out, u8 = case
    maps = G.make_maps(seed, shapes, u8)
    exp = torch.from_numpy(golden[f"map_{name}_expected"])
    got = resize_maps(maps, out, dtype=torch.float64).cpu()
    assert got.shape == exp.shape
    tol = 1e-6 * exp.abs().max().item()
    assert (got - exp).abs().max().item() <= tol
    got32 = resize_maps(maps, out).cpu()
    assert got32.dtype == torch.float32 and torch.equal(got32, got.float())
    # uint8 transport == the same maps as float32
    if u8:
        assert torch.equal(resize_maps([m.astype(np.float32) for m in maps], out, dtype=torch.float64).cpu(), got)
    # the datasets' normalisations, float64 arithmetic
    for norm, eps in (("max", 0.0), ("max_eps", 1e-7)):
        e = torch.stack([x / (x.max() + eps) for x in exp])
        g = resize_maps(maps, out, normalise=norm, eps=eps, dtype=torch.float64).cpu()
        assert (g - e).abs().max().item() <= 1e-6


def test_all_zero_maps_nan_for_air_zero_for_coco():
    from scanpaths_amd.transforms import attention_maps
    z = [np.zeros((48, 64), np.float32), np.ones((30, 40), np.float32)]
    air = attention_maps(z, (30, 40)).cpu()
    assert air.shape == (2, 1, 30, 40) and torch.isnan(air[0]).all() and torch.equal(air[1], torch.ones(1, 30, 40))
    coco = attention_maps(z, (30, 40), eps=1e-7).cpu()
    assert torch.equal(coco[0], torch.zeros(1, 30, 40)) and torch.equal(coco[1], torch.full((1, 30, 40), np.float32(1 / (1 + 1e-7))))


def test_detector_boxes_rasterised_on_the_device_equal_the_host_map():
    from scanpaths_amd.dataset import detector_box_map
    from scanpaths_amd.transforms import attention_maps, attention_maps_from_detections
    rng = np.random.Generator(np.random.PCG64(41))
    cats = ["cup", "fork", "tv"]
    sizes = [(320, 512), (427, 640), (100, 50), (320, 512)]
    dets, tasks = [], []
    for b, (h, w) in enumerate(sizes):
        ds = []
        for _ in range(int(rng.integers(0, 6)) if b else 0):
            x0, y0 = rng.uniform(0, w), rng.uniform(0, h)
            ds.append({"category": cats[int(rng.integers(0, 3))], "bbox": [x0, y0, x0 + rng.uniform(1, w), y0 + rng.uniform(1, h)]})
        dets.append(ds)
        tasks.append(cats[b % 3])
    got = attention_maps_from_detections(dets, tasks, sizes)
    host = [detector_box_map(d, t, s) for d, t, s in zip(dets, tasks, sizes)]
    assert torch.equal(got, attention_maps(host, (30, 40), eps=1e-7))
    assert torch.equal(got[0], torch.zeros_like(got[0]))


def _scene_records(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    recs = []
    for b in range(n):
        h, w = (480, 640) if b % 2 else (333, 500)
        objs = {}
        for i in range(7):
            objs[f"o{i}"] = {"x": int(rng.integers(0, w)), "y": int(rng.integers(0, h)), "h": int(rng.integers(1, h)),
                             "w": int(rng.integers(1, w))}
        q = {f"q{k}": f"o{int(rng.integers(0, 7))}" for k in range(int(rng.integers(0, 6)))}
        a = {f"a{k}": f"o{int(rng.integers(0, 7))}" for k in range(int(rng.integers(0, 6)))}
        recs.append({"height": h, "width": w, "objects": objs, "annotations": {"question": q, "fullAnswer": a}})
    return recs


def test_scene_graph_maps_equal_host_drawing_then_resize():
    from scanpaths_amd.transforms import resize_maps, scene_graph_maps
    recs = _scene_records(51, 4)
    got = scene_graph_maps(recs, (240, 320))
    for key in ("question", "fullAnswer"):
        maps, masks = [], np.zeros((len(recs), 5), np.float32)
        for b, f in enumerate(recs):            # get_scene_graph_info's drawing (AiR/dataset/dataset.py:76-90)
            pos = np.zeros((f["height"], f["width"], 5), np.float32)
            for idx, name in enumerate(f["annotations"][key].values()):
                o = f["objects"][name]
                pos[o["y"]:o["y"] + o["h"], o["x"]:o["x"] + o["w"], idx] = 1
                masks[b, idx] = 1
            maps.append(pos)
        assert torch.equal(got[f"{key}_objects_pos"], resize_maps(maps, (240, 320)))
        assert torch.equal(got[f"{key}_objects_masks"].cpu(), torch.from_numpy(masks))
    assert got["question_objects_pos"].shape == (4, 240, 320, 5)


def test_collate_raw_matches_host_built_batch_and_forward(golden):
    from scanpaths_amd.dataset import collate_func, collate_raw
    from scanpaths_amd.models.baseline_attention import baseline
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.transforms import resize_maps
    rng = np.random.Generator(np.random.PCG64(61))
    B, T = 3, 4
    sizes = [(480, 640), (600, 800), (240, 320)]
    imgs = G.make_images(62, sizes)
    boxes = G.make_maps(63, sizes, True)
    fix = []
    for b, (h, w) in enumerate(sizes):
        n = int(rng.integers(2, 7))
        ts = np.sort(rng.uniform(0, 3000, 2 * n)).reshape(n, 2)
        fix.append({"X": rng.uniform(0, w, n).tolist(), "Y": rng.uniform(0, h, n).tolist(), "T_start": ts[:, 0].tolist(),
                    "T_end": ts[:, 1].tolist(), "height": h, "width": w, "subject_answer": "yes", "answer": "yes" if b else "no"})
    samples = [{"image": imgs[b], "fixation": fix[b], "box_map": boxes[b], "img_name": f"i{b}", "question_id": f"q{b}"}
               for b in range(B)]
    raw = collate_raw(samples, max_length=T, size=(240, 320))
    # the host-built batch: images from the golden path (Pillow + torch-CPU float32), maps from resize + / max
    exp_imgs = torch.from_numpy(G.torchvision_images(imgs, (240, 320))) if _has_pil() else None
    am = resize_maps(boxes, (30, 40), dtype=torch.float64).cpu()
    host = collate_func([{"image": (exp_imgs[b] if exp_imgs is not None else raw["images"][b].cpu()), "fixation": fix[b],
                          "attention_map": (am[b] / am[b].max()).float()[None].numpy(), "img_name": f"i{b}",
                          "question_id": f"q{b}"} for b in range(B)], max_length=T)
    assert set(raw) == set(host)
    for k in host:
        if isinstance(host[k], torch.Tensor):
            assert torch.equal(raw[k], host[k]), k
        else:
            assert raw[k] == host[k], k
    model = baseline(convLSTM_length=T)
    fill_module(model, seed=5)
    model = model.cuda().eval()
    with torch.no_grad():
        a = model(raw["images"], raw["attention_maps"], raw["performances"])
        b = model(host["images"], host["attention_maps"], host["performances"])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _has_pil():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False
