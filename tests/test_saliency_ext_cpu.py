"""CPU-only checks of the shuffled AUC / CC / SIM / information gain layer: the new entry points are declared, bound and exported with
equal signatures; the numpy checker (tests/saliency_ext_ref.py) satisfies the identities its formulae imply; every argument refusal
of the Python layer is raised before a device or the library is touched."""
import inspect

import numpy as np
import pytest

import abi
import saliency_ext_ref as R

NEW = {"sp_fixation_pool_counts": ("int", 9), "sp_saliency_scores": ("int", 19)}


def test_new_entry_points_are_declared_bound_and_exported():
    abi.assert_declared(NEW, prefixes=("sp_saliency_metrics_",), allowed=("sp_saliency_metrics_lds_fixations",))


def _maps(g, shape, levels=None):
    S = g.uniform(0, 1, shape)
    if levels:
        S = np.floor(S * levels) / levels
    F = (g.uniform(0, 1, shape) < 0.05).astype(np.float64)
    w = g.integers(0, 4, shape) * (g.uniform(0, 1, shape) < 0.3)
    return S, F, w


def test_checker_identities():
    g = np.random.Generator(np.random.PCG64(5))
    S, F, w = _maps(g, (12, 16))
    # every positive above every pool value: 1; a constant map: 0.5
    hi = np.where(F > 0, S + 2.0, S)
    assert R.sauc(hi, F, np.where(F > 0, 0, w), brute=True) == 1.0
    assert R.sauc(np.full_like(S, 0.25), F, w, brute=True) == 0.5
    # sorted form == brute force, plain and under heavy ties (9 levels), positives inside the pool included
    for levels in (None, 9, 9, 9):
        S, F, w = _maps(g, (12, 16), levels)
        assert levels is None or len(np.unique(S)) <= 9
        v = R.sauc(S, F, w, brute=True)
        assert 0.0 <= v <= 1.0
    assert np.isnan(R.sauc(S, np.zeros_like(F), w, brute=True)) and np.isnan(R.sauc(S, F, np.zeros_like(w), brute=True))
    Sn = S.copy()
    Sn[3, 3] = np.nan
    assert np.isnan(R.sauc(Sn, F, w, brute=True))
    # pool weights: the pixels fixated on other images, weighted by how many other-image maps fixated them
    Fs = (g.uniform(0, 1, (5, 6, 8)) < 0.3).astype(np.float64)
    cls = [0, 1, 0, 2, 1]
    cnt, tot = R.pool_counts(Fs, cls, 3)
    wts = R.pool_weights(cnt, tot, cls)
    for k in range(5):
        assert np.array_equal(wts[k], sum((Fs[h] > 0).astype(np.int64) for h in range(5) if cls[h] != cls[k]))
    assert (wts >= 0).all() and np.array_equal(tot, (Fs > 0).sum(0))
    assert abs(R.cc(S, 3 * S + 1) - 1.0) <= 1e-14 and abs(R.cc(S, -S) + 1.0) <= 1e-14 and np.isnan(R.cc(S, np.ones_like(S)))
    assert abs(R.sim(S, S) - 1.0) <= 1e-14 and abs(R.sim(S, 7 * S) - 1.0) <= 1e-14
    assert np.isnan(R.sim(S, np.zeros_like(S))) and np.isnan(R.sim(Sn, S))
    for mix in (0.0, 0.01, 1.0):
        assert R.infogain(S, F, S, mix) == 0.0                      # exactly: the two sides are the same numbers
    assert R.infogain(S, F, np.ones_like(S), 0.0) != 0.0 and R.infogain(S, F, np.ones_like(S), 1.0) == 0.0
    assert np.isnan(R.infogain(S, np.zeros_like(F), S, 0.0)) and np.isnan(R.infogain(S, F, np.zeros_like(S), 0.0))
    # a fixation on an exact zero of the prediction costs 52 bits against a uniform baseline's log2(1 / P) when nothing is mixed in
    Z = np.zeros((4, 4))
    Z[0, 0] = 1.0
    Fz = np.zeros((4, 4))
    Fz[3, 3] = 1.0
    assert abs(R.infogain(Z, Fz, np.ones((4, 4)), 0.0) - (-52.0 - np.log2(R.EPS + 1.0 / 16))) <= 1e-12


def test_public_surface_of_the_extra_metrics():
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import saliency_maps as S
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    assert M.EXTRA_METRICS == ("sAUC", "CC", "SIM", "IG")
    assert list(inspect.signature(M.AUC_shuffled).parameters) == ["saliencyMap", "fixationMap", "otherMap"]
    assert list(inspect.signature(M.CC).parameters) == list(inspect.signature(M.SIM).parameters) == ["saliencyMap", "densityMap"]
    p = inspect.signature(M.InfoGain).parameters
    assert list(p) == ["saliencyMap", "fixationMap", "baselineMap", "uniform_mix"]
    assert p["uniform_mix"].kind is inspect.Parameter.KEYWORD_ONLY and p["uniform_mix"].default is inspect.Parameter.empty
    p = inspect.signature(S.scanpath_saliency).parameters
    assert p["extra_metrics"].default == () and p["image_groups"].default is None and p["uniform_mix"].default is None
    assert p["baseline_sigma"].default is None
    for fn in (E.saliency_evaluation, E.saliency_human_evaluation, E.saliency_centre_prior_evaluation):
        p = inspect.signature(fn).parameters
        assert p["extra_metrics"].default == () and p["image_keys"].default is None and p["sigma"].default is inspect.Parameter.empty
    for fn in (M.saliency_scores_pairs, M.SIM, M.InfoGain, S.scanpath_saliency, E.saliency_evaluation):
        assert "min-max" in fn.__doc__, fn.__name__             # the docstrings say which normalisation is NOT applied


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import saliency_maps as S
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M

    def no_lib():
        raise AssertionError("validation must come first")

    def no_device():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(S, "_device", no_device)
    monkeypatch.setattr(M, "_device", no_device)
    monkeypatch.setattr(hip, "lib", no_lib)
    s, f = np.ones((6, 8)), np.zeros((6, 8))
    f[2, 3] = 1.0
    # information gain without uniform_mix, or with one outside [0, 1]
    with pytest.raises(TypeError):
        M.InfoGain(s, f, s)
    with pytest.raises(TypeError, match="uniform_mix"):
        M.saliency_scores_pairs(s[None], f[None], baseline_maps=s[None])
    for mix in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            M.InfoGain(s, f, s, uniform_mix=mix)
    # the other map holds counts
    for bad in (np.full((6, 8), 0.5), -np.ones((6, 8)), np.full((6, 8), np.nan)):
        with pytest.raises(ValueError, match="integers"):
            M.AUC_shuffled(s, f, bad)
    # shapes: no resizing
    with pytest.raises(ValueError):
        M.AUC_shuffled(s, f, np.ones((6, 9)))
    with pytest.raises(ValueError):
        M.CC(s, np.ones((3, 4)))
    with pytest.raises(ValueError):
        M.SIM(s, np.ones((8, 6)))
    with pytest.raises(ValueError):
        M.InfoGain(s, np.ones((6, 7)), s, uniform_mix=0.0)
    with pytest.raises(ValueError):
        M.InfoGain(s, f, np.ones((5, 8)), uniform_mix=0.0)
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s, f[None], density_maps=s[None])                              # [N,H,W] only
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s[None], f[None], density_maps=np.ones((2, 6, 8)))
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s[None], f[None], image_groups=[0, 1])                         # one image per map
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s[None], f[None], image_groups=[-1])
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s[None], f[None], other_maps=f[None], image_groups=[0])        # two pools
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s[None], None, image_groups=[0])                               # a pool without fixations
    with pytest.raises(ValueError):
        M.saliency_scores_pairs(s[None], f[None])                                              # nothing to score
    # scanpath level
    p = [np.array([[1.0, 2.0, 0.1]]), np.array([[3.0, 4.0, 0.2]])]
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], p, [0, 1], (240, 320), 2.0, extra_metrics=("sAUC", "AUC_Borji"))
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], p, [0, 1], (240, 320), 2.0, extra_metrics=("CC", "CC"))
    with pytest.raises(TypeError, match="uniform_mix"):
        S.scanpath_saliency(p, [0, 1], p, [0, 1], (240, 320), 2.0, extra_metrics=("IG",))
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], p, [0, 1], (240, 320), 2.0, extra_metrics=("sAUC",), image_groups=[0])
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], p, [0, 1], (240, 320), 2.0, extra_metrics=("sAUC",), image_groups=[0, -1])
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], p, [0, 1], (240, 320), 2.0, prediction="centre_prior")  # takes no predictions
    with pytest.raises(ValueError):
        S.scanpath_saliency(p, [0, 1], [], [], (240, 320), 2.0, prediction="uniform")
    # evaluation level: predicted keys and image keys
    with pytest.raises(ValueError, match="not among gt_keys"):
        E.saliency_evaluation(p, p, ["a", "b"], ["a", "c"], sigma=2.0, extra_metrics=("sAUC",))
    with pytest.raises(ValueError, match="two images"):
        E.saliency_evaluation(p + p, p, ["a", "b", "a", "b"], ["a", "b"], sigma=2.0, extra_metrics=("sAUC",),
                              image_keys=["i", "j", "j", "j"])
    with pytest.raises(ValueError):
        E.saliency_evaluation(p, p, ["a", "b"], ["a", "b"], sigma=2.0, extra_metrics=("sAUC",), image_keys=["i"])
    with pytest.raises(TypeError, match="uniform_mix"):
        E.saliency_evaluation(p, p, ["a", "b"], ["a", "b"], sigma=2.0, extra_metrics=("IG",))
    with pytest.raises(TypeError):
        E.saliency_human_evaluation(p, ["a", "a"])                                             # sigma is required
    with pytest.raises(ValueError, match="two images"):
        E.saliency_human_evaluation(p, ["a", "a"], sigma=2.0, image_keys=["i", "j"])
    with pytest.raises(TypeError, match="uniform_mix"):
        E.saliency_centre_prior_evaluation(p, ["a", "b"], sigma=2.0, extra_metrics=("IG",))
