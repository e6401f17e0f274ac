"""CPU-only checks of the fixation / density map layer (scanpaths_amd/utils/evaltools/saliency_maps.py): the host weight builder is
scipy's kernel bit for bit, arguments are validated before anything touches a device, the fixture holds numeric arrays only."""
import inspect
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_npz


def test_gaussian_weights_equal_scipy_bit_for_bit():
    pytest.importorskip("scipy")
    from scipy.ndimage import correlate1d
    from scanpaths_amd.utils.evaltools.saliency_maps import _half_kernel, gaussian_weights
    for sigma, truncate in [(10.0, 4.0), (1.5, 4.0), (2.5, 3.0), (0.3, 4.0), (7.7, 2.5), (12.0, 4.0), (20.0, 4.0), (1.0, 0.0)]:
        w = gaussian_weights(sigma, truncate)
        r = int(truncate * sigma + 0.5)
        assert w.shape == (2 * r + 1,)
        # scipy's own kernel, read off an impulse: gaussian_filter1d correlates with exactly these weights
        from scipy.ndimage import gaussian_filter1d
        imp = np.zeros(2 * r + 1)
        imp[r] = 1.0
        assert np.array_equal(gaussian_filter1d(imp, sigma, mode="constant", truncate=truncate), w), (sigma, truncate)
        assert np.array_equal(correlate1d(imp, w, mode="constant"), w)
        assert np.array_equal(_half_kernel(sigma, truncate), w[r:])
    assert np.array_equal(_half_kernel(0.0, 4.0), np.ones(1))


def test_public_surface_and_signatures():
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import saliency_maps as S
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    for name in ("fixation_maps", "density_maps", "scanpath_saliency"):
        assert getattr(M, name) is getattr(S, name)
    p = list(inspect.signature(S.fixation_maps).parameters)
    assert p[:5] == ["scanpaths", "groups", "frame_size", "output_shape", "weight"]
    assert inspect.signature(S.fixation_maps).parameters["weight"].default == "binary"
    sig = inspect.signature(S.density_maps)
    assert list(sig.parameters)[:5] == ["maps", "sigma", "truncate", "mode", "normalise"]
    assert sig.parameters["sigma"].default is inspect.Parameter.empty            # the library picks no visual angle
    assert (sig.parameters["truncate"].default, sig.parameters["mode"].default, sig.parameters["normalise"].default) == (4.0, "constant", None)
    sig = inspect.signature(S.scanpath_saliency)
    assert list(sig.parameters)[:9] == ["gt_scanpaths", "gt_groups", "pred_scanpaths", "pred_groups", "frame_size", "sigma",
                                        "output_shape", "mode", "pred_weight"]
    assert sig.parameters["sigma"].default is inspect.Parameter.empty and sig.parameters["pred_weight"].default == "count"
    sig = inspect.signature(E.saliency_evaluation)
    assert list(sig.parameters)[:5] == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "frame_size"]
    assert sig.parameters["frame_size"].default == (240, 320) and sig.parameters["sigma"].default is inspect.Parameter.empty
    assert list(inspect.signature(M.saliency_metrics_pairs).parameters) == ["saliency_maps", "fixation_maps", "jitter"]


def test_scanpath_rows_and_result_records():
    from scanpaths_amd.utils.evaltools.saliency_maps import _rows
    from scanpaths_amd.utils.evaluation import predict_results_fix_vectors
    fv = np.zeros(3, dtype={"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")})
    fv["start_x"], fv["start_y"], fv["duration"] = [1, 2, 3], [4, 5, 6], [0.1, 0.2, 0.3]
    assert np.array_equal(_rows(fv), np.array([[1, 4, 0.1], [2, 5, 0.2], [3, 6, 0.3]]))
    assert _rows(fv[:0]).shape == (0, 3) and _rows([]).shape[0] == 0 and _rows(np.zeros((0, 3))).shape == (0, 3)
    assert np.array_equal(_rows([[1, 2], [3, 4]]), np.array([[1.0, 2.0], [3.0, 4.0]]))
    with pytest.raises(ValueError):
        _rows(np.zeros((4, 1)))
    with pytest.raises(ValueError):
        _rows(np.zeros(2, dtype={"names": ("x", "y"), "formats": ("f8", "f8")}))
    fvs, keys = predict_results_fix_vectors([{"qid": "q7", "X": [1.0, 2.0], "Y": [3.0, 4.0], "T": [250.0, 500.0]},
                                             {"qid": 3, "X": [], "Y": [], "T": []}])
    assert keys == ["q7", 3] and np.array_equal(fvs[0], np.array([[1, 3, 0.25], [2, 4, 0.5]])) and fvs[1].shape == (0, 3)
    with pytest.raises(ValueError):
        predict_results_fix_vectors([{"qid": 1, "X": [1.0], "Y": [], "T": [2.0]}])


def test_argument_validation_happens_on_the_host(monkeypatch):
    """every refusal below is raised before a device or the library is needed: _device() is stubbed, hip.lib() would raise"""
    import torch
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import saliency_maps as S

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(S, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hip, "lib", no_lib)
    p = [np.array([[1.0, 2.0, 0.1]]), np.array([[3.0, 4.0, 0.2]])]
    with pytest.raises(ValueError):
        S.fixation_maps(p, [0], (240, 320))                                  # one group per scanpath
    with pytest.raises(ValueError):
        S.fixation_maps(p, [0, -1], (240, 320))
    with pytest.raises(ValueError):
        S.fixation_maps(p, [0, 2], (240, 320), num_groups=2)
    with pytest.raises(ValueError):
        S.fixation_maps(p, [0, 1], (240, 320), weight="median")
    with pytest.raises(ValueError):
        S.fixation_maps([q[:, :2] for q in p], [0, 1], (240, 320), weight="duration")
    with pytest.raises(ValueError):
        S.fixation_maps([p[0], p[1][:, :2]], [0, 1], (240, 320))              # mixed column counts
    with pytest.raises(ValueError):
        S.fixation_maps(p, [0, 1], (0, 320))
    with pytest.raises(ValueError):
        S.fixation_maps(p, [0, 1], (240, 320), output_shape=(0, 4))
    m = np.zeros((2, 6, 8))
    with pytest.raises(TypeError):
        S.density_maps(m)                                                    # sigma has no default
    for kw in (dict(sigma=2.0, mode="wrap"), dict(sigma=2.0, mode="mirror"), dict(sigma=-1.0), dict(sigma=(1.0, 2.0, 3.0)),
               dict(sigma=float("nan")), dict(sigma=2.0, normalise="l2"), dict(sigma=2.0, truncate=-1.0)):
        with pytest.raises(ValueError):
            S.density_maps(m, **kw)
    with pytest.raises(ValueError):
        S.density_maps(np.zeros((6, 8)), sigma=1.0)                           # [G,H,W] only
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], p, [0, 2], (240, 320), sigma=2.0)      # predicted group without a human one
    with pytest.raises(TypeError):
        E.saliency_evaluation(p, p, ["a", "b"], ["a", "b"])                   # sigma is required
    with pytest.raises(ValueError, match="not among gt_keys"):
        E.saliency_evaluation(p, p, ["a", "b"], ["a", "c"], sigma=2.0)
    with pytest.raises(ValueError):
        E.saliency_evaluation(p, p, ["a"], ["a", "a"], sigma=2.0)


def test_fixmaps_fixture_holds_numeric_arrays_only():
    d = load_npz(os.path.join(GOLDEN, "fixmaps.npz"))
    assert len(d) > 100
    for k, v in d.items():
        assert v.dtype.kind in "fiu", (k, v.dtype)
    for p in os.listdir(GOLDEN):
        if p.startswith("fixmaps"):
            assert os.path.getsize(os.path.join(GOLDEN, p)) < 1024 * 1024, p
    # what the generator promises to cover
    lens, grp = d["fm/len"], d["fm/group"]
    assert (lens == 0).any() and lens.max() > 64 and 3 not in set(grp.tolist()) and grp.max() == 4
    assert np.isnan(d["fm/fix"]).any() and (d["fm/fix"][:, 0] == d["fm/frame"][1]).any() and d["fm/0/count"].max() >= 2
    assert sum(k.endswith("/auc") for k in d) >= 6 and all(d[k] >= 1e-9 for k in d if k.endswith("/gap"))
