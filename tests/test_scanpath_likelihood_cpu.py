"""CPU-only checks of the scanpath-likelihood layer: the two entry points are declared, bound and exported with equal
signatures and refuse bad arguments before any launch; the Python checker (tests/scanpath_likelihood_ref.py) holds the answers worked
out by hand; the public signatures are the documented ones; every argument refusal of the Python layer is raised before a device or the
library is touched."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import abi
import scanpath_likelihood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sp_scan_likelihood_max_cells": ("int", 0), "sp_scan_likelihood": ("int", 29)}
LOG2E = 1.0 / math.log(2.0)


def test_new_entry_points_are_declared_bound_and_exported():
    from scanpaths_amd.utils.evaltools import scanpath_likelihood as M
    lib = abi.assert_declared(NEW, prefixes=("sp_scan_likelihood_",))
    assert lib.sp_scan_likelihood_max_cells() == M.MAX_CELLS == R.MAX_CELLS == 2048
    assert lib.sp_scan_max_fixations() == M.MAX_FIXATIONS == R.MAX_FIXATIONS == 64
    assert "scanlik.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()


# the arguments of sp_scan_likelihood by position
PROBS, MU, S2, BASE, BROWS, FIX, START, COUNT, RFIRST, RN, ORDER, NR, NT, HM, WM, NS, NCOL, FW, FH, U = range(20)
LL, IG, NSS, AUC, DLL, CONT, TERM, DROPPED, STREAM = range(20, 29)


def test_launcher_refuses_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too.  Every call below is a refused one."""
    call = abi.raw_lib().sp_scan_likelihood
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")
    ok = [p] * 11 + [2, 4, 30, 40, 5, 3, 320.0, 240.0, 0.01] + [p] * 8 + [None]

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[globals()[k]] = v
        return call(*a)

    for k in (PROBS, FIX, START, COUNT, RFIRST, RN, ORDER):
        assert call(*[None if i == k else a for i, a in enumerate(ok)]) == -2, k
    none = dict(LL=None, IG=None, NSS=None, AUC=None, DLL=None, CONT=None, TERM=None, DROPPED=None)
    assert with_(**none) == -2                                      # every output NULL
    assert with_(BASE=None) == -2 and with_(BROWS=None) == -2       # IG without its baseline
    assert with_(MU=None) == -2 and with_(S2=None) == -2            # DLL without its parameters
    # a bad scalar is refused whichever outputs are asked for: here IG and DLL are not, so their inputs may be NULL
    few = dict(IG=None, DLL=None, BASE=None, BROWS=None, MU=None, S2=None)
    for k, bad in (("NR", 0), ("NR", -1), ("NT", 0), ("NT", -2), ("HM", 0), ("WM", 0), ("WM", -40), ("NS", 0), ("NS", -1), ("NCOL", 1),
                   ("NCOL", 0), ("FW", 0.0), ("FW", -1.0), ("FW", nan), ("FW", inf), ("FH", 0.0), ("FH", nan), ("FH", inf), ("U", -0.01),
                   ("U", 1.0), ("U", 1.5), ("U", nan), ("U", inf)):
        assert with_(**{k: bad}) == -1, (k, bad)
        assert with_(**dict(few, **{k: bad})) == -1, (k, bad)
    assert with_(HM=2049, WM=1) == -1 and with_(HM=32, WM=65) == -1 and with_(HM=1 << 16, WM=1 << 16) == -1     # beyond max_cells
    assert with_(NCOL=2) == -1                                      # DLL needs the duration column
    assert with_(MU=None, NCOL=2) == -2                             # NULL is answered before a bad scalar


def _one(p, fix, frame=(10.0, 10.0), shape=None, **kw):
    """one row, one step, one fixation"""
    p = np.asarray(p, dtype=np.float32)
    shape = shape or (1, len(p) - 1)
    res = R.scanpath_likelihood(p[None, None], [np.array([fix], dtype=np.float64)], [0], frame, shape, **kw)
    return {k: v.reshape(-1)[0] for k, v in res.items()}


def test_checker_values_by_hand_spatial():
    P = 20
    res = _one([0.2] + [0.04] * P, (3.0, 3.0), shape=(4, 5))                               # a uniform map
    assert res["LL"] == 0.0 and np.isnan(res["NSS"]) and res["AUC"] == 0.5 and res["n"] == 1 and res["dropped"] == 0
    # one cell at 0.7, the rest equal, the fixation on the peak (cell 7 of a 4 x 5 map: row 1, col 2)
    rest = np.float32(0.2 / (P - 1))
    p = np.full(1 + P, rest, dtype=np.float32)
    p[0], p[1 + 7] = 0.1, 0.7
    res = _one(p, (5.0, 3.0), shape=(4, 5))
    hi, lo = float(np.float32(0.7)), float(rest)
    Z = hi + (P - 1) * lo
    assert res["AUC"] == 1.0
    assert abs(res["LL"] - math.log2(P * hi / Z)) <= 1e-14
    # closed form of the ddof-1 deviation of one value hi among P - 1 values lo: (hi - lo) / sqrt(P); NSS = (hi - mean) / std
    nss = (hi - Z / P) / ((hi - lo) / math.sqrt(P))
    assert abs(res["NSS"] - nss) <= 1e-12 * nss
    off = _one(p, (0.5, 0.5), shape=(4, 5))                                               # a fixation on one of the equal cells
    assert off["AUC"] == 0.5 * (P - 2) / (P - 1) and off["NSS"] < 0 < res["NSS"]
    # the mixture: u moves q towards 1 / P
    mixed = _one(p, (5.0, 3.0), shape=(4, 5), uniform_mix=0.25)
    assert abs(mixed["LL"] - math.log2(P * (0.75 * hi / Z + 0.25 / P))) <= 1e-14
    # an unnormalised row scores as its normalised one
    assert abs(_one(p * np.float32(4.0), (5.0, 3.0), shape=(4, 5))["LL"] - res["LL"]) <= 1e-14


def test_checker_values_by_hand_information_gain_and_zeros():
    g = np.random.default_rng(2)
    P = 12
    p = g.uniform(0.01, 1.0, 1 + P).astype(np.float32)
    same = p[1:].astype(np.float64)[None]
    for u in (0.0, 0.05):
        res = _one(p, (7.0, 4.0), shape=(3, 4), uniform_mix=u, baseline=same, baseline_rows=[0])
        assert res["IG"] == 0.0                                                           # a baseline equal to the map
        res = _one(p, (7.0, 4.0), shape=(3, 4), uniform_mix=u, baseline=np.full((1, P), 3.0), baseline_rows=[0])
        assert abs(res["IG"] - res["LL"]) <= 1e-14                                        # against uniform, IG is LL
    assert np.isnan(_one(p, (7.0, 4.0), shape=(3, 4), baseline=np.zeros((1, P)), baseline_rows=[0])["IG"])    # baseline sum 0
    p[1 + 5] = 0.0                                                                        # cell 5 of 3 x 4: row 1, col 1
    res = _one(p, (3.0, 4.0), shape=(3, 4), uniform_mix=0.0, baseline=same, baseline_rows=[0])
    assert res["LL"] == -np.inf and res["IG"] == -np.inf                                  # no epsilon: reported as such
    res = _one(p, (3.0, 4.0), shape=(3, 4), uniform_mix=0.125)
    assert abs(res["LL"] - math.log2(0.125)) <= 1e-14                                   # log2(P * u / P)


def test_checker_values_by_hand_duration_stop_and_drops():
    for mu, s2 in ((-1.2, 0.3), (0.4, 2.0)):
        got = R.duration_log2_density(math.exp(mu), mu, s2)
        assert abs(got - -(mu + 0.5 * math.log(2 * math.pi * s2)) * LOG2E) <= 1e-14
    for d, s2 in ((0.0, 1.0), (-0.2, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.3, 0.0), (0.3, -1.0)):
        assert np.isnan(R.duration_log2_density(d, 0.0, s2)), (d, s2)
    # the loss's own form (models/loss.py MLPLogNormalDistribution without its epsilon), times log2 e
    d, mu, s2 = 0.27, -1.1, 0.4
    nll = math.log(d) + 0.5 * math.log(2 * math.pi * s2) + (math.log(d) - mu) ** 2 / (2 * s2)
    assert abs(R.duration_log2_density(d, mu, s2) + nll * LOG2E) <= 1e-14
    # STOP: T = 4 steps with p_0 = 1/2, 1/4, 1/8, 1/16 of a total of 1
    T, P = 4, 6
    probs = np.zeros((1, T, 1 + P), dtype=np.float32)
    for t in range(T):
        probs[0, t, 0] = 0.5 ** (t + 1)
        probs[0, t, 1:] = (1.0 - 0.5 ** (t + 1)) / P
    cont = [math.log2(1.0 - 0.5 ** (t + 1)) for t in range(T)]
    term = [-(t + 1.0) for t in range(T)]
    paths = [np.full((n, 2), 1.0) for n in (0, 1, 2, 3, 4, 7)]
    res = R.scanpath_likelihood(probs, paths, [0] * 6, (4.0, 4.0), (2, 3), min_length=2)
    assert np.allclose(res["CONT"][0], cont, rtol=0, atol=1e-7) and np.allclose(res["TERM"][0], term, rtol=0, atol=1e-7)
    c, t = res["CONT"][0], res["TERM"][0]
    want = [-np.inf, -np.inf, t[2], c[2] + t[3], c[2] + c[3], c[2] + c[3]]                  # n < min_length (twice), = min_length, < T, = T, > T
    assert res["STOP"].tolist() == want and res["n"].tolist() == [0, 1, 2, 3, 4, 4]
    assert R.scanpath_likelihood(probs, paths[:1], [0], (4.0, 4.0), (2, 3), min_length=0)["STOP"][0] == t[0]      # the empty scanpath
    assert R.scanpath_likelihood(probs[:, :1], paths[1:2], [0], (4.0, 4.0), (2, 3), min_length=3)["STOP"][0] == 0.0   # n' = T < min_length
    # drops: NaN in the spatial outputs, a DLL all the same; the frame's last pixel is inside, x = w is not
    fix = np.array([(3.999, 3.999, 0.2), (4.0, 1.0, 0.2), (-0.1, 1.0, 0.2), (1.0, float("nan"), 0.2)])
    res = R.scanpath_likelihood(probs, [fix], [0], (4.0, 4.0), (2, 3), mu=np.zeros((1, T)), sigma2=np.ones((1, T)),
                                baseline=np.ones((1, P)), baseline_rows=[0])
    assert res["dropped"][0] == 3 and res["n"][0] == 4 and R.cell_of(3.999, 3.999, (4.0, 4.0), (2, 3)) == 5
    for m in ("LL", "IG", "NSS", "AUC"):
        assert np.isnan(res[m][0]).tolist() == [m == "NSS", True, True, True], m            # (the maps here are constant: no NSS)
    assert not np.isnan(res["DLL"][0]).any()


def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import scanpath_likelihood as M
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as V
    assert M.METRICS == R.METRICS == ("LL", "IG", "NSS", "AUC", "DLL", "STOP")
    assert V.scanpath_likelihood is M.scanpath_likelihood and V.cell_baselines is M.cell_baselines
    p = inspect.signature(M.scanpath_likelihood).parameters
    assert list(p) == ["probs", "scanpaths", "rows", "frame_size", "uniform_mix", "metrics", "map_shape", "baseline", "baseline_rows",
                       "log_normal_mu", "log_normal_sigma2", "min_length"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    assert p["uniform_mix"].default is None and p["metrics"].default == ("LL", "NSS", "AUC") and p["min_length"].default == 0
    assert all(p[k].default is None for k in ("map_shape", "baseline", "baseline_rows", "log_normal_mu", "log_normal_sigma2"))
    assert list(inspect.signature(M.cell_baselines).parameters) == ["scanpaths", "image_groups", "frame_size", "map_shape"]
    p = inspect.signature(E.likelihood_evaluation).parameters
    assert list(p) == ["predict", "fix_vectors", "keys", "performances", "image_keys", "baseline", "uniform_mix", "metrics", "min_length",
                       "frame_size", "map_shape"]
    assert p["uniform_mix"].kind is inspect.Parameter.KEYWORD_ONLY and p["uniform_mix"].default is inspect.Parameter.empty
    assert all(p[k].default is None for k in ("performances", "image_keys", "baseline", "map_shape"))
    assert p["metrics"].default == ("LL", "NSS", "AUC") and p["min_length"].default == 0 and p["frame_size"].default == (240, 320)
    assert list(inspect.signature(E.LikelihoodTable.add).parameters) == ["self", "means"]
    assert list(inspect.signature(E.LikelihoodTable.result).parameters) == ["self"]
    p = inspect.signature(inference.run_likelihood_loop).parameters
    assert list(p) == ["model", "loader", "uniform_mix", "metrics", "min_length", "baseline", "ablate_attention_info", "frame_size",
                       "map_shape"]
    assert p["uniform_mix"].kind is inspect.Parameter.KEYWORD_ONLY and p["uniform_mix"].default is inspect.Parameter.empty
    assert p["baseline"].default is None and p["ablate_attention_info"].default is False


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import scanpath_likelihood as M

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M, "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    T, Hm, Wm = 4, 3, 5
    probs = torch.full((2, T, 1 + Hm * Wm), 1.0 / 16)
    mu, s2 = torch.zeros(2, T), torch.ones(2, T)
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3]])
    frame, kw = (24, 32), dict(map_shape=(Hm, Wm), uniform_mix=0.01)
    base = np.ones((3, Hm * Wm))
    call = M.scanpath_likelihood
    with pytest.raises(ValueError, match="unknown"):
        call(probs, [sp], [0], frame, metrics=("LL", "SS"), **kw)
    with pytest.raises(ValueError, match="repeated"):
        call(probs, [sp], [0], frame, metrics=("AUC", "AUC"), **kw)
    with pytest.raises(ValueError, match="no likelihood metric"):
        call(probs, [sp], [0], frame, metrics=(), **kw)
    for m in ("LL", "IG"):
        with pytest.raises(TypeError, match="uniform_mix"):
            call(probs, [sp], [0], frame, metrics=(m,), map_shape=(Hm, Wm), baseline=base, baseline_rows=[0])
    for u in (-0.1, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="uniform_mix"):
            call(probs, [sp], [0], frame, map_shape=(Hm, Wm), uniform_mix=u)
        with pytest.raises(ValueError, match="uniform_mix"):
            E.likelihood_evaluation({"all_actions_prob": probs}, [[sp], [sp]], ["a", "b"], uniform_mix=u, map_shape=(Hm, Wm))
    for ml in (-1, 1.5, True):
        with pytest.raises(ValueError, match="min_length"):
            call(probs, [sp], [0], frame, metrics=("STOP",), min_length=ml, **kw)
    with pytest.raises(TypeError, match="baseline"):
        call(probs, [sp], [0], frame, metrics=("IG",), **kw)
    with pytest.raises(TypeError, match="baseline"):
        call(probs, [sp], [0], frame, metrics=("IG",), baseline=base, **kw)
    with pytest.raises(TypeError, match="log_normal"):
        call(probs, [sp], [0], frame, metrics=("DLL",), log_normal_mu=mu, **kw)
    with pytest.raises(ValueError, match="columns"):
        call(probs, [sp[:, :2]], [0], frame, metrics=("DLL",), log_normal_mu=mu, log_normal_sigma2=s2, **kw)
    with pytest.raises(ValueError, match="log_normal"):
        call(probs, [sp], [0], frame, metrics=("DLL",), log_normal_mu=mu[:1], log_normal_sigma2=s2[:1], **kw)
    with pytest.raises(ValueError, match="baseline of shape"):
        call(probs, [sp], [0], frame, metrics=("IG",), baseline=np.ones((3, 14)), baseline_rows=[0], **kw)
    for bad in ([3], [-1]):
        with pytest.raises(ValueError, match="out of range"):
            call(probs, [sp], [0], frame, metrics=("IG",), baseline=base, baseline_rows=bad, **kw)
    with pytest.raises(ValueError, match="one baseline row per scanpath"):
        call(probs, [sp, sp], [0, 1], frame, metrics=("IG",), baseline=base, baseline_rows=[0], **kw)
    for bad in ([2], [-1]):
        with pytest.raises(ValueError, match="out of range"):
            call(probs, [sp], bad, frame, **kw)
    with pytest.raises(ValueError, match="one row per scanpath"):
        call(probs, [sp, sp], [0], frame, **kw)
    with pytest.raises(ValueError, match="kernel limit"):
        call(probs, [np.zeros((M.MAX_FIXATIONS + 1, 2))], [0], frame, **kw)
    with pytest.raises(ValueError, match="map_shape is required"):
        call(probs, [sp], [0], frame, uniform_mix=0.01)
    for shape in ((4, 4), (3, 6), (0, 15), (-3, -5)):
        with pytest.raises(ValueError, match="map_shape"):
            call(probs, [sp], [0], frame, uniform_mix=0.01, map_shape=shape)
    with pytest.raises(ValueError, match="kernel limit"):
        call(torch.zeros(1, 1, 2050), [sp], [0], frame, uniform_mix=0.01, map_shape=(1, 2049))
    with pytest.raises(ValueError, match="probs"):
        call(probs[0], [sp], [0], frame, **kw)
    with pytest.raises(ValueError, match="probs"):
        call(probs.numpy(), [sp], [0], frame, **kw)
    for bad in ((0, 32), (24, float("inf")), (float("nan"), 32)):
        with pytest.raises(ValueError, match="frame_size"):
            call(probs, [sp], [0], bad, **kw)
    # the default map shape belongs to 1201 actions; an empty scanpath list: empty arrays, no device
    res = call(torch.zeros(2, T, 1201), [], [], (240, 320), uniform_mix=0.0, metrics=("LL", "STOP"))
    assert list(res) == ["LL", "STOP", "n", "dropped"] and res["LL"].shape == (0, T) and res["STOP"].shape == (0,)
    assert res["n"].dtype == res["dropped"].dtype == np.int32 and res["LL"].dtype == np.float64
    # evaluation level
    one = {"all_actions_prob": probs}
    two = {"good_all_actions_prob": probs, "poor_all_actions_prob": probs}
    fv = [[sp, sp], [sp]]
    ev = E.likelihood_evaluation
    with pytest.raises(TypeError):
        ev(one, fv, ["a", "b"], map_shape=(Hm, Wm))                                    # uniform_mix is required
    with pytest.raises(ValueError, match="one key per sample"):
        ev(one, fv, ["a"], **kw)
    with pytest.raises(ValueError, match="one performance per subject"):
        ev(two, fv, ["a", "b"], [[True], [False]], **kw)
    with pytest.raises(ValueError, match="predict lacks 'good_all_actions_prob'"):
        ev(one, fv, ["a", "b"], [[True, False], [False]], **kw)
    with pytest.raises(ValueError, match="predict lacks 'all_actions_prob'"):
        ev(two, fv, ["a", "b"], **kw)
    with pytest.raises(ValueError, match="predict lacks 'log_normal_mu'"):
        ev(one, fv, ["a", "b"], metrics=("DLL",), **kw)
    with pytest.raises(ValueError, match="samples"):
        ev(one, fv + [[sp]], ["a", "b", "c"], **kw)
    with pytest.raises(ValueError, match="image_keys is required"):
        ev(one, fv, ["a", "b"], baseline=base, metrics=("IG",), **kw)
    with pytest.raises(ValueError, match="one image key"):
        ev(one, fv, ["a", "b"], image_keys=[0], baseline=base, metrics=("IG",), **kw)
    with pytest.raises(ValueError, match="out of range"):
        ev(one, fv, ["a", "b"], image_keys=[0, 3], baseline=base, metrics=("IG",), **kw)
    with pytest.raises(TypeError, match="baseline"):
        ev(one, fv, ["a", "b"], metrics=("IG",), **kw)
    with pytest.raises(ValueError, match="unknown"):
        ev(one, fv, ["a", "b"], metrics=("SS",), **kw)
    means, per_key = ev(one, [[], []], ["a", "b"], metrics=("LL", "STOP"), **kw)           # no scanpaths at all: NaN tables, no device
    assert per_key["keys"] == ["a", "b"] and np.isnan(per_key["LL"]).all() and np.isnan(per_key["STOP"]).all()
    assert np.isnan(means["LL"]) and means["LL_count"] == 0 and means["LL_nan_keys"] == 2 and means["dropped"] == 0
    table = E.LikelihoodTable()
    table.add(means)
    assert np.isnan(table.result()["LL"]) and table.result()["STOP_count"] == 0


def test_cell_baselines_needs_a_device(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import scanpath_likelihood as M
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M.cell_baselines([np.array([[1.0, 1.0]])], [0], (24, 32), (3, 4))
    with pytest.raises(hip.HipError, match="no CPU path"):
        M.scanpath_likelihood(torch.zeros(1, 2, 13), [np.array([[1.0, 1.0]])], [0], (24, 32), uniform_mix=0.0, map_shape=(3, 4))
