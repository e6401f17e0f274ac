"""CPU-only checks of the search-efficiency layer: the two entry points are declared, bound and exported with equal
signatures and refuse bad arguments before any launch; every argument refusal of the Python layer is raised before a device or the
library is touched; the Python checker (tests/search_efficiency_ref.py) holds answers worked out by hand and, for T = 3 on a 2 x 2 map,
equals the exhaustive enumeration of all 5^3 action sequences under the sampler's rule in exact rational arithmetic -- which makes the
checker independent of the closed form's own reasoning."""
import inspect
import itertools
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi
import search_efficiency_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sp_scan_target_hits": ("int", 11), "sp_scan_target_mass": ("int", 16)}


def test_new_entry_points_are_declared_bound_and_exported():
    from scanpaths_amd.utils.evaltools import search_efficiency as M
    lib = abi.assert_declared(NEW, prefixes=("sp_scan_target_",))
    assert lib.sp_scan_max_fixations() == M.MAX_FIXATIONS == R.MAX_FIXATIONS == 64
    assert M.MAX_SIDE == R.MAX_SIDE == 1024
    assert "scansearch.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()


def test_launchers_refuse_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too.  Every call below is a refused one."""
    lib = abi.raw_lib()
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")
    # sp_scan_target_hits(fix, ncol, start, count, box, nscan, max_steps, hit, path, spr, stream)
    ok = [p, 2, p, p, p, 5, 6, p, p, p, None]
    hits = lib.sp_scan_target_hits

    def with_(call, base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)

    for k in (0, 2, 3, 4):
        assert with_(hits, ok, **{f"a{k}": None}) == -2, k
    assert with_(hits, ok, a7=None, a8=None, a9=None) == -2         # every output NULL
    for k, bad in ((1, 1), (1, 0), (1, -2), (5, 0), (5, -1), (6, 0), (6, -3)):
        assert with_(hits, ok, **{f"a{k}": bad}) == -1, (k, bad)
        assert with_(hits, ok, a8=None, a9=None, **{f"a{k}": bad}) == -1, (k, bad)        # whichever outputs are asked for
    assert with_(hits, ok, a0=None, a1=1) == -2                     # NULL is answered before a bad scalar
    # sp_scan_target_mass(probs, box, box_row, R, T, Hm, Wm, NB, frame_w, frame_h, min_length, MASS, HIT, TFP, cells, stream)
    ok = [p, p, p, 3, 4, 30, 40, 5, 320.0, 240.0, 2, p, p, p, p, None]
    mass = lib.sp_scan_target_mass
    for k in (0, 1, 2):
        assert with_(mass, ok, **{f"a{k}": None}) == -2, k
    assert with_(mass, ok, a11=None, a12=None, a13=None, a14=None) == -2
    for k, bad in ((3, 0), (3, -1), (4, 0), (4, -2), (5, 0), (5, -30), (5, 1025), (6, 0), (6, 1025), (6, 1 << 20), (7, 0), (7, -1),
                   (8, 0.0), (8, -1.0), (8, nan), (8, inf), (9, 0.0), (9, -2.0), (9, nan), (9, inf), (10, -1)):
        assert with_(mass, ok, **{f"a{k}": bad}) == -1, (k, bad)
        assert with_(mass, ok, a11=None, a12=None, a14=None, **{f"a{k}": bad}) == -1, (k, bad)
    assert with_(mass, ok, a1=None, a3=0) == -2                     # NULL is answered before a bad scalar


def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import search_efficiency as M
    empty = inspect.Parameter.empty
    p = inspect.signature(M.target_hits).parameters
    assert list(p) == ["scanpaths", "boxes", "max_steps"] and p["max_steps"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["max_steps"].default is empty
    p = inspect.signature(M.target_hit_probability).parameters
    assert list(p) == ["probs", "boxes", "box_rows", "frame_size", "min_length", "map_shape"]
    assert p["min_length"].kind is inspect.Parameter.KEYWORD_ONLY and p["min_length"].default is empty and p["map_shape"].default is None
    p = inspect.signature(E.search_efficiency_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "boxes", "max_steps", "image_keys"]
    assert p["max_steps"].kind is inspect.Parameter.KEYWORD_ONLY and p["max_steps"].default is empty and p["image_keys"].default is None
    p = inspect.signature(E.search_efficiency_human_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "gt_keys", "boxes", "max_steps", "image_keys"] and p["max_steps"].default is empty
    p = inspect.signature(E.search_efficiency_model_evaluation).parameters
    assert list(p)[:7] == ["predict", "keys", "boxes", "min_length", "max_steps", "performances", "human_curve"]
    assert p["min_length"].kind is inspect.Parameter.KEYWORD_ONLY and p["min_length"].default is empty and p["max_steps"].default is empty
    assert p["performances"].default is None and p["human_curve"].default is None
    p = inspect.signature(inference.run_search_efficiency_loop).parameters
    assert list(p)[:5] == ["model", "loader", "boxes", "min_length", "max_steps"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is empty for k in ("boxes", "min_length", "max_steps"))
    assert list(inspect.signature(E.SearchEfficiencyTable.add).parameters) == ["self", "means"]
    assert list(inspect.signature(E.LikelihoodTable.result).parameters) == ["self"]               # the older table stays as it is


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import search_efficiency as M

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M, "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3]])
    box = [0.0, 0.0, 4.0, 4.0]
    hits = M.target_hits
    with pytest.raises(TypeError):
        hits([sp], [box])                                                                  # max_steps has no default
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_steps"):
            hits([sp], [box], max_steps=bad)
    with pytest.raises(ValueError, match="kernel limit"):
        hits([np.zeros((M.MAX_FIXATIONS + 1, 2))], [box], max_steps=6)                      # a scanpath of 65
    with pytest.raises(ValueError, match="one box per scanpath"):
        hits([sp, sp], [box], max_steps=6)
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        hits([sp], [[0.0, 0.0, 4.0]], max_steps=6)
    for v in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="non-finite box"):
            hits([sp], [[0.0, v, 4.0, 4.0]], max_steps=6)
    with pytest.raises(ValueError, match="scanpath is an"):
        hits([np.zeros((3, 1))], [box], max_steps=6)
    res = hits([], np.zeros((0, 4)), max_steps=3)                                          # nothing to score: empty arrays, no device
    assert res["hit"].dtype == np.int32 and res["hit"].shape == (0,) and res["SPR"].shape == (0,) and res["n"].shape == (0,)

    T, Hm, Wm = 4, 3, 5
    probs = torch.full((2, T, 1 + Hm * Wm), 1.0 / 16)
    frame, kw = (24, 40), dict(map_shape=(Hm, Wm), min_length=1)
    prob = M.target_hit_probability
    with pytest.raises(TypeError):
        prob(probs, [box], [0], frame, map_shape=(Hm, Wm))                                 # min_length has no default
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_length"):
            prob(probs, [box], [0], frame, map_shape=(Hm, Wm), min_length=bad)
    with pytest.raises(ValueError, match="probs"):
        prob(probs[0], [box], [0], frame, **kw)
    with pytest.raises(ValueError, match="probs"):
        prob(probs.numpy(), [box], [0], frame, **kw)
    with pytest.raises(ValueError, match="map_shape is required"):
        prob(probs, [box], [0], frame, min_length=1)
    for shape in ((4, 4), (3, 6), (0, 15), (-3, -5)):
        with pytest.raises(ValueError, match="map_shape"):
            prob(probs, [box], [0], frame, min_length=1, map_shape=shape)
    with pytest.raises(ValueError, match="kernel limit"):
        prob(torch.zeros(1, 1, 1026), [box], [0], frame, min_length=1, map_shape=(1, 1025))
    for bad in ((0, 32), (24, float("inf")), (float("nan"), 32)):
        with pytest.raises(ValueError, match="frame_size"):
            prob(probs, [box], [0], bad, **kw)
    with pytest.raises(ValueError, match="non-finite box"):
        prob(probs, [[0.0, 0.0, float("nan"), 4.0]], [0], frame, **kw)
    for bad in ([2], [-1]):
        with pytest.raises(ValueError, match="out of range"):
            prob(probs, [box], bad, frame, **kw)
    with pytest.raises(ValueError, match="one row per box"):
        prob(probs, [box, box], [0], frame, **kw)
    # no cell limit: the 40 x 64 map is accepted (the default map shape belongs to 1201 actions); without boxes there is no device call
    res = prob(torch.zeros(2, T, 2561), np.zeros((0, 4)), [], (320, 512), min_length=1, map_shape=(40, 64))
    assert res["TFP"].shape == (0, T) and res["cells"].dtype == np.int32
    assert prob(torch.zeros(2, T, 1201), [], [], (240, 320), min_length=0)["MASS"].shape == (0, T)

    # evaluation level
    boxes = {"a": box, "b": box}
    ev = E.search_efficiency_evaluation
    with pytest.raises(TypeError):
        ev([sp], [sp], ["a"], ["a"], boxes)
    with pytest.raises(ValueError, match="max_steps"):
        ev([sp], [sp], ["a"], ["a"], boxes, max_steps=0)
    with pytest.raises(ValueError, match="one key per fixation vector"):
        ev([sp, sp], [sp], ["a"], ["a"], boxes, max_steps=3)
    with pytest.raises(ValueError, match="not among gt_keys"):
        ev([sp], [sp], ["a"], ["b"], boxes, max_steps=3)
    with pytest.raises(ValueError, match="'c'.*has no box"):
        ev([sp, sp], [sp], ["a", "c"], ["a"], boxes, max_steps=3)                           # a key without a box: an error, not a drop
    with pytest.raises(ValueError, match="has no box"):
        E.search_efficiency_human_evaluation([sp], ["c"], boxes, max_steps=3)
    with pytest.raises(ValueError, match="two images"):
        ev([sp, sp], [sp], ["a", "a"], ["a"], boxes, max_steps=3, image_keys=["i", "j"])
    with pytest.raises(ValueError, match="non-finite box"):
        ev([sp], [sp], ["a"], ["a"], {"a": [0.0, 0.0, float("inf"), 1.0]}, max_steps=3)
    one = {"all_actions_prob": probs}
    two = {"good_all_actions_prob": probs, "poor_all_actions_prob": probs}
    mv = E.search_efficiency_model_evaluation
    mkw = dict(min_length=1, max_steps=3, frame_size=frame, map_shape=(Hm, Wm))
    with pytest.raises(TypeError):
        mv(one, ["a", "b"], boxes, max_steps=3)
    with pytest.raises(ValueError, match="has no box"):
        mv(one, ["a", "c"], boxes, **mkw)
    with pytest.raises(ValueError, match="predict lacks 'good_all_actions_prob'"):
        mv(one, ["a", "b"], boxes, performances=[[True], [False]], **mkw)
    with pytest.raises(ValueError, match="predict lacks 'all_actions_prob'"):
        mv(two, ["a", "b"], boxes, **mkw)
    with pytest.raises(ValueError, match="one list of performances per sample"):
        mv(two, ["a", "b"], boxes, performances=[[True]], **mkw)
    with pytest.raises(ValueError, match="samples"):
        mv(one, ["a", "b", "a"], boxes, **mkw)
    with pytest.raises(ValueError, match="human_curve"):
        mv(one, ["a", "b"], boxes, human_curve=[0.1, 0.2], **mkw)


def test_no_cpu_path(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import search_efficiency as M
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M.target_hits([np.array([[1.0, 1.0]])], [[0.0, 0.0, 2.0, 2.0]], max_steps=2)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M.target_hit_probability(torch.zeros(1, 2, 13), [[0.0, 0.0, 2.0, 2.0]], [0], (24, 32), min_length=0, map_shape=(3, 4))


def test_curve_helpers():
    from scanpaths_amd.utils.evaltools import search_efficiency as M
    hit = [0, 2, -1, 5, 2, 1, -1, 0]
    curve = M.search_curve(hit, 4)
    assert curve.tolist() == [2 / 8, 3 / 8, 5 / 8, 5 / 8] == R.search_curve(hit, 4).tolist()     # a hit at 5 is beyond 4 steps
    assert M.hit_counts(hit, 4).tolist() == [2.0, 3.0, 5.0, 5.0]
    assert M.tfp_auc(curve) == 2 / 8 + 3 / 8 + 5 / 8 + 5 / 8
    assert M.probability_mismatch(curve, [0.5, 0.25, 0.625, 1.0]) == 0.25 + 0.125 + 0.0 + 0.375
    assert np.isnan(M.search_curve([], 3)).all()
    with pytest.raises(ValueError, match="equal lengths"):
        M.probability_mismatch(curve, curve[:3])


def test_checker_hits_by_hand():
    box = (10.0, 10.0, 20.0, 30.0)                                                        # centre (15, 20)
    paths = [np.array([(3.0, 4.0), (6.0, 8.0), (10.0, 10.0), (15.0, 15.0)]),              # hit at 2: on x_min and y_min, inside
             np.array([(12.0, 12.0), (0.0, 0.0)]),                                        # hit at 0
             np.array([(20.0, 15.0), (15.0, 30.0), (0.0, 0.0)]),                          # on x_max, on y_max: outside, never hits
             np.array([(0.0, 0.0), (float("nan"), 1.0), (15.0, 15.0)]),                   # NaN before the hit
             np.array([(0.0, 20.0), (15.0, 20.0), (float("nan"), 1.0)]),                  # NaN after the hit
             np.zeros((0, 2))]
    res = R.target_hits(paths, [box] * 6, 3)
    assert res["hit"].tolist() == [2, 0, -1, 2, 1, -1] and res["n"].tolist() == [3, 2, 3, 3, 3, 0]
    assert res["path"][0] == 5.0 + math.sqrt(20.0) and res["SPR"][0] == 20.0 / (5.0 + math.sqrt(20.0))     # |(3,4) - (15,20)| = 20
    assert res["path"][1] == 0.0 and res["SPR"][1] == 1.0
    assert np.isnan(res["path"][[2, 3, 5]]).all() and np.isnan(res["SPR"][[2, 3, 5]]).all()
    assert res["path"][4] == 15.0 and res["SPR"][4] == 1.0
    assert R.target_hits(paths[:1], [box], 2)["hit"][0] == -1                            # the hit lies just beyond max_steps
    far = np.array([(0.0, 20.0), (15.0, 20.0)])                                           # the near edge of a wide box: centre (105, 20)
    assert R.target_hits([far], [(10.0, 10.0, 200.0, 30.0)], 2)["SPR"][0] == 105.0 / 15.0  # a ratio above 1 is not clipped
    assert R.target_hits([np.zeros((65, 2))], [(-1.0, -1.0, 1.0, 1.0)], 3)["hit"][0] == -1   # beyond the limit: nothing is read


def test_checker_mass_by_hand():
    # a uniform map: a box of k cells has m = k / P wherever no terminate mass enters
    Hm, Wm, T = 4, 5, 3
    P = Hm * Wm
    probs = np.full((1, T, 1 + P), 0.25, dtype=np.float32)
    frame = (40.0, 50.0)                                                                  # centres 5, 15, .. on both axes
    boxes = [(10.0, 10.0, 30.0, 40.0), (0.0, 0.0, 50.0, 40.0), (0.0, 0.0, 5.0, 5.0), (20.0, 0.0, 10.0, 40.0), (1e300, 0.0, 2e300, 40.0)]
    res = R.target_mass(probs, boxes, [0] * 5, frame, (Hm, Wm), min_length=T)
    assert res["cells"].tolist() == [6, P, 0, 0, 0]                                       # (an edge ON a centre: 5 < 5 is false)
    assert (res["MASS"][0] == 6 / P).all() and (res["MASS"][1] == 1.0).all()
    assert (res["MASS"][2:] == 0).all() and (res["HIT"][2:] == 0).all() and (res["TFP"][2:] == 0).all()      # empty boxes: all zeros
    assert res["TFP"][1].tolist() == [1.0, 1.0, 1.0] and res["HIT"][1].tolist() == [1.0, 0.0, 0.0]
    k = 6 / P
    assert np.allclose(res["TFP"][0], [1 - (1 - k) ** (t + 1) for t in range(T)], rtol=0, atol=1e-15)
    # the whole frame with terminate mass: TFP_t = 1 - prod_{s <= t} (1 - m_s - q_s) in closed form, here with m + q = 1 from
    # min_length on (every continuing scanpath hits) and m = 1 before it
    g = np.random.default_rng(0)
    probs = g.uniform(0.01, 1.0, (1, 4, 1 + P)).astype(np.float32)
    res = R.target_mass(probs, [(0.0, 0.0, 50.0, 40.0)], [0], frame, (Hm, Wm), min_length=2)
    assert res["TFP"][0].tolist() == [1.0, 1.0, 1.0, 1.0] and res["cells"][0] == P
    res = R.target_mass(probs, [(0.0, 0.0, 50.0, 40.0)], [0], frame, (Hm, Wm), min_length=0)
    p0, Z = probs[0, :, 0].astype(np.float64), probs[0, :, 1:].astype(np.float64).sum(1)
    assert np.allclose(res["TFP"][0], Z[0] / (Z[0] + p0[0]), rtol=0, atol=1e-15)          # hit at step 0 or terminated at step 0
    # a partial box with terminate mass, against the product form
    box = [(0.0, 0.0, 30.0, 20.0)]                                                        # columns 0..2 of rows 0..1
    res = R.target_mass(probs, box, [0], frame, (Hm, Wm), min_length=1)
    cellsum = np.array([sum(float(probs[0, t, 1 + r * Wm + c]) for r in range(2) for c in range(3)) for t in range(4)])
    D = np.where(np.arange(4) >= 1, Z + p0, Z)
    m, q = cellsum / D, np.where(np.arange(4) >= 1, p0 / D, 0.0)
    surv = np.cumprod(1 - m - q)
    want_hit = np.r_[1.0, surv[:-1]] * m
    assert res["cells"][0] == 6 and np.allclose(res["MASS"][0], m, rtol=0, atol=1e-15)
    assert np.allclose(res["HIT"][0], want_hit, rtol=0, atol=1e-15) and np.allclose(res["TFP"][0], np.cumsum(want_hit), rtol=0, atol=1e-15)
    # a step without mass before min_length: NaN from there on; p_0 = 1 from min_length on: the scanpath ends, later steps add nothing
    probs[0, 1, 1:] = 0.0
    res = R.target_mass(probs, box, [0], frame, (Hm, Wm), min_length=2)
    assert np.isnan(res["TFP"][0]).tolist() == [False, True, True, True] and np.isnan(res["MASS"][0, 2])
    probs[0, 1, 0] = 1.0
    res = R.target_mass(probs, box, [0], frame, (Hm, Wm), min_length=1)
    assert res["HIT"][0, 1:].tolist() == [0.0, 0.0, 0.0] and res["TFP"][0, 3] == res["TFP"][0, 0]
    assert R.target_mass(probs, box, [7], frame, (Hm, Wm), min_length=1)["cells"][0] == -1   # a row that does not exist


def test_checker_pixel_is_the_fused_one():
    """the sampler's kernel evaluates (float)k * g + 0.5f * g as ONE fused multiply-add; where k * g is inexact in float32 the unfused
    value differs by an ulp.  The checker (and the kernel) take the fused value; on power-of-two granularities both agree."""
    for n, frame in ((40, 320), (30, 240), (64, 512), (40, 320), (9, 100)):
        assert R.centres(n, frame) == R.centres(n, frame, fused=False), (n, frame)
    fused, plain = R.centres(7, 75), R.centres(7, 75, fused=False)
    differ = [k for k in range(7) if fused[k] != plain[k]]
    assert len(differ) == 1 and abs(fused[differ[0]] - plain[differ[0]]) == float(np.spacing(np.float32(min(fused[differ[0]], plain[differ[0]]))))
    assert R.centres(30, 240) == [8.0 * k + 4.0 for k in range(30)]
    # an edge exactly on a centre, on both sides: x_min on it keeps the cell, x_max on it leaves it out
    c = R.centres(9, 100)
    assert R.cell_range(9, 100, c[3], c[6]) == (3, 6) and R.cell_range(9, 100, np.nextafter(c[3], 1e9), np.nextafter(c[6], 1e9)) == (4, 7)
    assert R.cell_range(9, 100, -1e300, 1e300) == (0, 9) and R.cell_range(9, 100, 50.0, 40.0) == (0, 0)
    assert R.cell_range(9, 100, 100.0, 1e300) == (0, 0) and R.cell_range(9, 100, float("nan"), 50.0) == (0, 0)


def test_checker_equals_the_exhaustive_enumeration():
    """T = 3, a 2 x 2 map, min_length = 1: all 5^3 action sequences under the sampler's rule (terminate masked at step 0, the first
    terminate ends the scanpath) in exact rational arithmetic; the probability that the first fixation inside the box is fixation t is
    summed and compared with the checker's HIT, absolutely, to 1e-12.  (Sums of at most 2048 non-negative terms carry a relative error
    <= 2048 * 2^-53 = 2.3e-13 in any order; the recursion multiplies factors <= 1 over T <= 16 steps.)"""
    T, Hm, Wm, min_length = 3, 2, 2, 1
    frame = (20.0, 20.0)                                                                  # centres 5, 15
    g = np.random.default_rng(11)
    probs = g.uniform(0.05, 1.0, (2, T, 5)).astype(np.float32)                            # unnormalised on purpose
    boxes = [(0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 20.0, 10.0), (10.0, 0.0, 20.0, 20.0), (0.0, 0.0, 20.0, 20.0), (7.0, 7.0, 9.0, 9.0),
             (0.0, 10.0, 10.0, 20.0)]
    rows = [0, 1, 0, 1, 0, 1]
    res = R.target_mass(probs, boxes, rows, frame, (Hm, Wm), min_length)
    assert res["cells"].tolist() == [1, 2, 2, 4, 0, 1]
    for b, (box, row) in enumerate(zip(boxes, rows)):
        pixel = {a: (((a - 1) % Wm + 0.5) * frame[1] / Wm, ((a - 1) // Wm + 0.5) * frame[0] / Hm) for a in range(1, 5)}
        member = {a for a, (x, y) in pixel.items() if box[0] <= x < box[2] and box[1] <= y < box[3]}
        first = [Fraction(0)] * T
        total = Fraction(0)
        for seq in itertools.product(range(5), repeat=T):
            w = Fraction(1)
            for t, a in enumerate(seq):
                allowed = range(1, 5) if t < min_length else range(5)
                if a not in allowed:
                    w = Fraction(0)
                    break
                w *= Fraction(float(probs[row, t, a])) / sum(Fraction(float(probs[row, t, k])) for k in allowed)
            if not w:
                continue
            total += w
            for t, a in enumerate(seq):
                if a == 0:
                    break                                                                 # the first terminate ends the scanpath
                if a in member:
                    first[t] += w
                    break
        assert total == 1
        for t in range(T):
            assert abs(res["HIT"][b, t] - float(first[t])) <= 1e-12, (b, t, res["HIT"][b, t], float(first[t]))
            assert abs(res["TFP"][b, t] - float(sum(first[:t + 1]))) <= 1e-12, (b, t)
