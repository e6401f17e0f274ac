"""CPU-only: the host half of scanpaths_amd.transforms.  Pillow's fixed-point BILINEAR tables built by the host, run through a numpy
restatement of Pillow's two 8-bit passes, equal Pillow's own resize on a sweep of size pairs (where PIL imports); the Gaussian
weights equal scipy's (where scipy imports); the transforms fixture holds numeric arrays only; wrong inputs are refused before any
device is touched."""
import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_npz

SIZE_PAIRS = [((480, 640), (320, 512)), ((600, 800), (240, 320)), ((1050, 1680), (320, 512)), ((37, 53), (320, 512)),
              ((1, 1), (5, 7)), ((1, 9), (4, 3)), ((13, 17), (13, 17)), ((29, 31), (7, 40)), ((240, 320), (1, 1)),
              ((101, 7), (33, 7)), ((7, 101), (7, 33)), ((3, 2), (11, 300)), ((255, 257), (256, 254))]


def pillow_resize_numpy(img: np.ndarray, size):
    """Pillow's ImagingResample for 8-bit RGB, BILINEAR: horizontal pass into uint8 (only when the width changes), then vertical"""
    from scanpaths_amd.transforms import PRECISION_BITS, pil_bilinear_coeffs
    H, W = size
    x = img.astype(np.int64)

    def one_pass(x, axis, out):
        _, bounds, kk = pil_bilinear_coeffs(x.shape[axis], out)
        xt = np.moveaxis(x, axis, 0)
        acc = np.full((out,) + xt.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for o in range(out):
            lo, n = bounds[o]
            for i in range(n):
                acc[o] += xt[lo + i] * int(kk[o, i])
        return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255), 0, axis)

    if x.shape[1] != W:
        x = one_pass(x, 1, W)
    if x.shape[0] != H:
        x = one_pass(x, 0, H)
    return x.astype(np.uint8)


@pytest.mark.parametrize("src,dst", SIZE_PAIRS)
def test_fixed_point_tables_restate_pillow_bilinear(src, dst):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(sum(src) * 1000 + sum(dst)))
    img = rng.integers(0, 256, size=src + (3,), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
    got = pillow_resize_numpy(img, dst)
    assert np.array_equal(got, ref), (src, dst, np.abs(got.astype(int) - ref).max())


def test_coefficient_rows_sum_to_one_in_fixed_point():
    from scanpaths_amd.transforms import pil_bilinear_coeffs
    for n_in, n_out in [(480, 320), (640, 512), (1680, 512), (5, 300), (1, 9)]:
        ksize, bounds, kk = pil_bilinear_coeffs(n_in, n_out)
        assert (bounds[:, 0] >= 0).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ksize).all()
        assert (np.abs(kk.sum(1) - (1 << 22)) <= ksize).all()


def test_gaussian_weights_equal_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    from scanpaths_amd.transforms import antialias_sigma, gaussian_half_kernel
    for n_in, n_out in [(480, 30), (640, 40), (600, 240), (105, 32), (30, 30), (10, 40)]:
        s = antialias_sigma(n_in, n_out)
        half = gaussian_half_kernel(s)
        if s <= 1e-15:
            assert half.tolist() == [1.0]
            continue
        R = half.size - 1
        delta = np.zeros(2 * R + 1)
        delta[R] = 1.0
        full = ndimage.gaussian_filter1d(delta, s, mode="constant", truncate=4.0)     # the kernel itself, from scipy
        assert np.array_equal(full[R:], half) and np.array_equal(full[:R + 1][::-1], half)


def test_fixture_holds_numeric_arrays_only():
    d = load_npz(GOLDEN + "/transforms.npz")
    assert len(d) >= 10
    for k, v in d.items():
        assert v.dtype.kind in "fiub", (k, v.dtype)


def test_wrong_inputs_are_refused_before_the_device():
    from scanpaths_amd import transforms as T
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(TypeError):
        T.resize_normalise_images([img.astype(np.float32)], (4, 4))
    with pytest.raises(ValueError):
        T.resize_normalise_images([np.zeros((8, 8, 4), np.uint8)], (4, 4))
    with pytest.raises(ValueError):
        T.resize_normalise_images([np.zeros((0, 8, 3), np.uint8)], (4, 4))
    with pytest.raises(ValueError):
        T.resize_normalise_images([], (4, 4))
    with pytest.raises(ValueError):
        T.resize_normalise_images([img], 4)
    with pytest.raises(ValueError):
        T.resize_normalise_images([img], (0, 4))
    with pytest.raises(TypeError):
        T.resize_normalise_images([torch.zeros(8, 8, 3)], (4, 4))
    with pytest.raises(TypeError):
        T.resize_maps([np.zeros((8, 8), np.float64)], (4, 4))
    with pytest.raises(ValueError):
        T.resize_maps([np.zeros((8,), np.float32)], (4, 4))
    with pytest.raises(ValueError):
        T.resize_maps([np.zeros((8, 8), np.float32), np.zeros((8, 8, 2), np.float32)], (4, 4))
    with pytest.raises(TypeError):
        T.resize_maps([np.zeros((8, 8), np.float32), np.zeros((8, 8), np.uint8)], (4, 4))
    with pytest.raises(ValueError):
        T.resize_maps([np.zeros((8, 8), np.float32)], (4, 4), normalise="sum")
    with pytest.raises(ValueError):
        T.resize_maps([], (4, 4))
    with pytest.raises(ValueError):
        T.attention_maps_from_detections([[]], ["cup", "fork"], (8, 8))
    with pytest.raises(ValueError):
        T.attention_maps([np.zeros((8, 8, 2), np.float32)], (4, 4))
    rec = {"height": 8, "width": 8, "objects": {str(i): {"x": 0, "y": 0, "h": 1, "w": 1} for i in range(6)},
           "annotations": {"question": {str(i): str(i) for i in range(6)}, "fullAnswer": {}}}
    with pytest.raises(ValueError):
        T.scene_graph_maps([rec])


def test_valid_calls_raise_hip_error_off_the_device():
    from scanpaths_amd import hip, transforms as T
    cpu = torch.device("cpu")
    with pytest.raises(hip.HipError):
        T.resize_normalise_images([np.zeros((8, 8, 3), np.uint8)], (4, 4), device=cpu)
    with pytest.raises(hip.HipError):
        T.resize_maps([np.zeros((8, 8), np.float32)], (4, 4), device=cpu)
    with pytest.raises(hip.HipError):
        T.attention_maps_from_detections([[]], ["cup"], (8, 8), device=cpu)
    if not torch.cuda.is_available():
        with pytest.raises(hip.HipError):
            T.resize_normalise_images([np.zeros((8, 8, 3), np.uint8)], (4, 4))
