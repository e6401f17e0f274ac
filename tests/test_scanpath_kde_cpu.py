"""CPU-only checks of the KDE baseline / gold-standard layer: the restatement tests/scanpath_kde_ref.py holds the answers
worked out by hand and its plain loops agree with its quick form; the entry points are declared, bound and exported and refuse bad
arguments before any launch; every Python refusal is raised before a device or the library is touched; information_gain_explained and a
LikelihoodTable merge of "GOLD" entries on made-up means; and the measurement the GPU tests' bar rests on: how far a serial and a
lane-strided-plus-butterfly summation of the same kernel values differ on the shared inputs (printed; DESIGN.md §20 records it)."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import scanpath_kde_cases as C
import abi
import scanpath_kde_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sp_scan_kde_max_bandwidths": ("int", 0), "sp_scan_kde": ("int", 26)}


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_one_by_two_map_by_hand():
    """frame 2 x 4, cells centred at x = 1 and 3; bandwidth 1: a source at x = 1 weighs its own cell 1 / (1 + e^-2), the other e^-2 / (1 + e^-2)"""
    frame, shape = (2.0, 4.0), (1, 2)
    near, far = 1.0 / (1.0 + math.exp(-2.0)), math.exp(-2.0) / (1.0 + math.exp(-2.0))
    near3, far3 = 1.0 / (1.0 + math.exp(-3.0)), math.exp(-3.0) / (1.0 + math.exp(-3.0))      # a source at x = 3.5: exponents -3.125, -0.125
    k = R.cell_kernel(1.0, 1.0, frame, shape, 1.0)
    assert np.abs(k - [[near, far]]).max() <= 1e-15
    paths, groups = [np.array([[1.0, 1.0]]), np.array([[3.0, 0.5]]), np.array([[1.0, 1.5], [3.5, 1.0]])], [0, 1, 1]
    for fn in (R.leave_out, R.quick_leave_out):
        res = fn(paths, groups, frame, shape, 1.0, 0.0, "image")
        assert res["others"].tolist() == [[3, 0], [1, 0], [1, 1]] and res["n"].tolist() == [1, 1, 2] and res["dropped"].tolist() == [0, 0, 0]
        # the fixation of image 0 (cell 0) under the three sources of image 1; those of image 1 under the one of image 0
        want = [[math.log2(2 * (far + near + far3) / 3), np.nan], [math.log2(2 * far), np.nan], [math.log2(2 * near), math.log2(2 * far)]]
        assert np.allclose(res["LL"], want, rtol=0, atol=1e-14, equal_nan=True)
        res = fn(paths, groups, frame, shape, 1.0, 0.25, "scanpath")
        assert res["others"].tolist() == [[0, 0], [2, 0], [1, 1]]
        # scanpath 1 (x = 3, cell 1) under the two fixations of scanpath 2: x = 1 weighs cell 1 far, x = 3.5 weighs it near3
        assert abs(res["LL"][1, 0] - math.log2(2 * (0.75 * ((far + near3) / 2) + 0.125))) <= 1e-14
        assert np.isnan(res["LL"][0]).all() and not np.isnan(res["LL"][2]).any()
        res = fn(paths, groups, frame, shape, 1.0, 0.0, "scanpath_step")
        assert res["others"].tolist() == [[0, 0], [1, 0], [1, 0]]                     # step 1 of scanpath 2 has no partner
        assert abs(res["LL"][1, 0] - math.log2(2 * far)) <= 1e-14 and np.isnan(res["LL"][2, 1])
    base = R.baselines(paths, groups, frame, shape, 1.0)
    assert base.shape == (2, 2) and np.abs(base[1] - [near, far]).max() <= 1e-15
    assert np.abs(base[0] - (np.array([far, near]) + R.cell_kernel(1.0, 1.5, frame, shape, 1.0)[0]
                             + R.cell_kernel(3.5, 1.0, frame, shape, 1.0)[0])).max() <= 1e-14
    assert (R.baselines(paths[:1], [0], frame, shape, 1.0) == 0.0).all()              # one image: exactly zero


def test_bandwidth_limits_and_unit_rows():
    for shape in ((3, 5), (8, 8), (30, 40)):
        paths, groups, frame = C.case(shape, big=False)
        q = R.Quick(paths, groups, frame, shape)
        for b in C.bandwidths(shape):
            wx, wy = q.weights(b)
            k = (wy[q.ok][:, :, None] * wx[q.ok][:, None, :]).reshape(int(q.ok.sum()), -1)
            assert np.abs(k.sum(1) - 1.0).max() <= 4e-16 * shape[0] * shape[1], (shape, b)      # every k_j sums to 1
        # bandwidth 1e-3: one-hot kernels of the NEAREST centre, so the table is the cell histogram of the other images -- without
        # image 3, whose fixations on a cell border lie between two centres and weigh each 1/2
        keep = [i for i, g in enumerate(groups) if g != C.IDS["two"]]
        q = R.Quick([paths[i] for i in keep], [groups[i] for i in keep], frame, shape)
        hist = np.zeros((q.G, shape[0] * shape[1]))
        np.add.at(hist, (q.g[q.ok], (q.row * shape[1] + q.col)[q.ok]), 1.0)
        assert (q.baselines(1e-3) == hist.sum(0, keepdims=True) - hist).all()
        # bandwidth 1e6: every kernel is 1 / P to within 1e-7, so 0 bits
        for leave in R.LEAVE:
            ll = q.leave_out(1e6, 0.0, leave)["LL"]
            assert np.abs(ll[~np.isnan(ll)]).max() <= 1e-6
    one = R.quick_leave_out(*C.case((1, 1))[:2], C.MAPS[1, 1], (1, 1), 3.0, 0.01, "scanpath")["LL"]
    assert np.abs(one[~np.isnan(one)]).max() <= 1e-15                                 # P = 1: every score 0


def test_plain_loops_equal_the_quick_form():
    shape = (3, 5)
    paths, groups, frame = C.case(shape, big=False)
    worst = 0.0
    for b, u, ml in ((1e-3, 0.0, None), (0.5, 0.01, 4), (10.0, 0.0, None), (45.3, 0.5, 16), (1e6, 0.01, 1)):
        assert np.abs(R.baselines(paths, groups, frame, shape, b, ml) - R.quick_baselines(paths, groups, frame, shape, b, ml)).max() <= 1e-12
        for leave in R.LEAVE:
            a = R.leave_out(paths, groups, frame, shape, b, u, leave, ml)
            q = R.quick_leave_out(paths, groups, frame, shape, b, u, leave, ml)
            for k in ("others", "n", "dropped"):
                assert a[k].dtype == q[k].dtype == np.int32 and (a[k] == q[k]).all(), (k, b, leave)
            assert (np.isnan(a["LL"]) == np.isnan(q["LL"])).all() and (np.isneginf(a["LL"]) == np.isneginf(q["LL"])).all()
            fin = np.isfinite(a["LL"])
            err = np.abs(a["LL"][fin] - q["LL"][fin]) / np.maximum(1.0, np.abs(a["LL"][fin]))
            worst = max(worst, float(err.max()))
    print(f"plain loops against the quick form: worst relative error {worst:.2e}")
    assert worst <= 1e-13
    s1 = R.search(paths, groups, frame, shape, [4.0, 8.0, 16.0], 0.01, "scanpath", quick=False)
    s2 = R.search(paths, groups, frame, shape, [4.0, 8.0, 16.0], 0.01, "scanpath", quick=True)
    assert s1["count"] == s2["count"] > 0 and s1["best"] == s2["best"] and np.abs(s1["LL"] - s2["LL"]).max() <= 1e-13


def test_summation_order_spread_on_the_shared_inputs():
    """serial against lane-strided-plus-butterfly summation of the same kernel values at the queries' cells, in bits: the room the GPU
    tests' bar 1e-12 * max(1, |ref|) has to leave for two correct summation orders"""
    worst = 0.0
    for shape in ((3, 5), (30, 40)):
        paths, groups, frame = C.case(shape, big=False)
        q = R.Quick(paths, groups, frame, shape)
        P = shape[0] * shape[1]
        for b in C.bandwidths(shape)[1:4]:
            wx, wy = q.weights(b)
            for i in np.flatnonzero(q.ok)[::7]:
                for member in (q.ok & (q.g != q.g[i]), q.ok & (q.g == q.g[i]) & (q.s != q.s[i])):
                    v = (wy[member, q.row[i]] * wx[member, q.col[i]]).tolist()
                    if not v:
                        continue
                    serial = 0.0
                    for x in v:
                        serial = serial + x
                    other = R.strided_butterfly_sum(v)
                    if serial > 0.0:
                        a, c = (math.log2(P * (0.99 * (s / len(v)) + 0.01 / P)) for s in (serial, other))
                        worst = max(worst, abs(a - c) / max(1.0, abs(a)))
    print(f"serial against lane-strided-plus-butterfly summation: worst difference {worst:.2e} of max(1, |bits|)")
    assert worst <= 1e-13                                                             # a factor of 10 under the bar


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    from scanpaths_amd.utils.evaltools import scanpath_kde as M
    lib = abi.assert_declared(NEW)
    assert lib.sp_scan_kde_max_bandwidths() == M.MAX_BANDWIDTHS == R.MAX_BANDWIDTHS >= 16
    assert lib.sp_scan_likelihood_max_cells() == M.MAX_CELLS == R.MAX_CELLS
    assert "scankde.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()


# the arguments of sp_scan_kde by position
FIX, PATH, STEP, IMG, ISTART, BLOCKS, N, NCOL, NG, NB, BW, NK, HM, WM, FW, FH, U, LEAVE, PREP, OWN, NOTHER, TABLES, LL, OTHERS, VALID = range(25)


def test_launcher_refuses_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too.  Every call below is a refused one."""
    call = abi.raw_lib().sp_scan_kde
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")
    good = (ctypes.c_double * 16)(*([8.0] * 16))
    bw = ctypes.addressof(good)

    def with_(leave, **kw):
        a = [p] * 6 + [10, 2, 2, 1, bw, 2, 30, 40, 320.0, 240.0, 0.01, leave] + [p] * 7 + [None]
        for k, v in kw.items():
            a[globals()[k]] = v
        return call(*a)

    for leave in (0, 1, 2):
        for k in ("FIX", "ISTART", "BW", "PREP"):
            assert with_(leave, **{k: None}) == -2, (leave, k)
    for k in ("OWN", "NOTHER", "TABLES", "IMG", "OTHERS", "VALID"):
        assert with_(0, **{k: None}) == -2, k
    for k in ("PATH", "STEP", "BLOCKS", "LL", "OTHERS", "VALID"):
        assert with_(1, **{k: None}) == -2 and with_(2, **{k: None}) == -2, k
    for leave in (0, 1, 2):
        for k, bad in (("NK", 0), ("NK", -1), ("NK", 17), ("HM", 0), ("WM", -40), ("N", -1), ("NG", -1), ("NB", -1), ("NCOL", 1), ("U", -0.01),
                       ("U", 1.0), ("U", nan), ("U", inf), ("FW", 0.0), ("FW", nan), ("FH", inf), ("FH", -1.0)):
            assert with_(leave, **{k: bad}) == -1, (leave, k, bad)
        assert with_(leave, HM=2049, WM=1) == -1 and with_(leave, HM=32, WM=65) == -1 and with_(leave, HM=1 << 16, WM=1 << 16) == -1
        for bad in (0.0, -1.0, nan, inf):
            for at in (0, 1):
                one = (ctypes.c_double * 16)(*([8.0] * 16))
                one[at] = bad
                assert with_(leave, BW=ctypes.addressof(one)) == -1, (leave, bad, at)
        assert with_(leave, FIX=None, NK=0) == -2                   # NULL is answered before a bad scalar
    assert with_(3) == -1 and with_(-1) == -1                       # leave: 0, 1 or 2
    assert with_(1, NG=0) == -1                                     # a pair pass needs an image


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import scanpath_kde as M
    assert M.LEAVE == R.LEAVE == ("image", "scanpath", "scanpath_step")
    p = inspect.signature(M.kde_cell_baselines).parameters
    assert list(p) == ["scanpaths", "image_groups", "frame_size", "map_shape", "bandwidth", "max_length"]
    assert p["bandwidth"].kind is inspect.Parameter.KEYWORD_ONLY and p["bandwidth"].default is inspect.Parameter.empty
    for fn, name in ((M.kde_leave_out_likelihood, "bandwidth"), (M.kde_bandwidth_search, "bandwidths")):
        p = inspect.signature(fn).parameters
        assert list(p) == ["scanpaths", "image_groups", "frame_size", "map_shape", name, "uniform_mix", "leave", "max_length"]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is inspect.Parameter.empty for k in (name, "uniform_mix", "leave"))
        assert p["max_length"].default is None
    p = inspect.signature(E.likelihood_gold_standard_evaluation).parameters
    assert list(p) == ["fix_vectors", "keys", "bandwidth", "uniform_mix", "max_length", "same_step", "frame_size", "map_shape"]
    assert all(p[k].default is inspect.Parameter.empty for k in ("bandwidth", "uniform_mix", "max_length"))
    assert p["same_step"].default is False and p["frame_size"].default == (240, 320) and p["map_shape"].default == (30, 40)
    assert list(inspect.signature(E.information_gain_explained).parameters) == ["means", "gold_means"]
    p = inspect.signature(inference.run_likelihood_gold_loop).parameters
    q = inspect.signature(inference.run_likelihood_loop).parameters
    assert list(p) == ["model", "loader", "gold_standard"] + list(q)[2:] and all(p[k].default == q[k].default for k in list(q)[2:])


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import scanpath_kde as M

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M, "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3]])
    args = ([sp, sp], [0, 1], (24, 32), (3, 4))
    kw = dict(uniform_mix=0.01, leave="image")
    for call, name in ((M.kde_leave_out_likelihood, "bandwidth"), (M.kde_bandwidth_search, "bandwidths")):
        with pytest.raises(TypeError):
            call(*args, **kw)                                                         # no default bandwidth
        with pytest.raises(TypeError):
            call(*args, **{name: 8.0}, leave="image")                                 # no default uniform_mix
        with pytest.raises(TypeError, match="uniform_mix"):
            call(*args, **{name: 8.0}, leave="image", uniform_mix=None)
        with pytest.raises(TypeError):
            call(*args, **{name: 8.0}, uniform_mix=0.01)                              # no default leave
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="bandwidth"):
                call(*args, **{name: bad}, **kw)
        for u in (-0.1, 1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="uniform_mix"):
                call(*args, **{name: 8.0}, leave="image", uniform_mix=u)
        with pytest.raises(ValueError, match="leave"):
            call(*args, **{name: 8.0}, uniform_mix=0.01, leave="subject")
        for ml in (0, -1, 1.5, True):
            with pytest.raises(ValueError, match="max_length"):
                call(*args, **{name: 8.0}, max_length=ml, **kw)
        with pytest.raises(ValueError, match="kernel limit"):
            call(args[0], args[1], (24, 32), (1, 2049), **{name: 8.0}, **kw)          # one cell more than 32 x 64
        with pytest.raises(ValueError, match="map_shape"):
            call(args[0], args[1], (24, 32), (0, 4), **{name: 8.0}, **kw)
        with pytest.raises(ValueError, match="frame_size"):
            call(args[0], args[1], (0, 32), (3, 4), **{name: 8.0}, **kw)
        with pytest.raises(ValueError, match="one image group per scanpath"):
            call(args[0], [0], (24, 32), (3, 4), **{name: 8.0}, **kw)
        with pytest.raises(ValueError, match="out of range"):
            call(args[0], [0, -1], (24, 32), (3, 4), **{name: 8.0}, **kw)
        with pytest.raises(ValueError):
            call([np.zeros((3, 1)), sp], [0, 1], (24, 32), (3, 4), **{name: 8.0}, **kw)   # a scanpath without a y column
    with pytest.raises(ValueError, match="bandwidths"):
        M.kde_bandwidth_search(*args, bandwidths=[], **kw)
    with pytest.raises(ValueError, match="bandwidths"):
        M.kde_bandwidth_search(*args, bandwidths=[2.0] * (M.MAX_BANDWIDTHS + 1), **kw)
    with pytest.raises(ValueError, match="one bandwidth"):
        M.kde_leave_out_likelihood(*args, bandwidth=[2.0, 4.0], **kw)
    with pytest.raises(TypeError):
        M.kde_cell_baselines(*args)
    with pytest.raises(ValueError, match="one bandwidth"):
        M.kde_cell_baselines(*args, bandwidth=[2.0, 4.0])
    for bad in (0.0, float("nan")):
        with pytest.raises(ValueError, match="bandwidth"):
            M.kde_cell_baselines(*args, bandwidth=bad)
    with pytest.raises(ValueError, match="kernel limit"):
        M.kde_cell_baselines(args[0], args[1], (24, 32), (2049, 1), bandwidth=8.0)
    # nothing to score: empty arrays, no device
    res = M.kde_leave_out_likelihood([], [], (24, 32), (3, 4), bandwidth=8.0, **kw)
    assert res["LL"].shape == (0, 0) and res["n"].shape == (0,) and res["others"].dtype == res["n"].dtype == res["dropped"].dtype == np.int32
    res = M.kde_leave_out_likelihood([np.zeros((0, 2))] * 2, [4, 9], (24, 32), (3, 4), bandwidth=8.0, **kw)
    assert res["LL"].shape == (2, 0) and res["n"].tolist() == [0, 0] and res["dropped"].tolist() == [0, 0]
    s = M.kde_bandwidth_search([], [], (24, 32), (3, 4), bandwidths=[4.0, 8.0], **kw)
    assert s["count"] == 0 and np.isnan(s["LL"]).all() and np.isnan(s["best"]) and s["bandwidths"].tolist() == [4.0, 8.0]
    # the keyed layer
    ev = E.likelihood_gold_standard_evaluation
    with pytest.raises(TypeError):
        ev([[sp, sp]], ["a"], bandwidth=8.0, uniform_mix=0.01)                        # max_length is required
    with pytest.raises(ValueError, match="max_length"):
        ev([[sp, sp]], ["a"], bandwidth=8.0, uniform_mix=0.01, max_length=None)
    with pytest.raises(ValueError, match="one key per sample"):
        ev([[sp, sp]], ["a", "b"], bandwidth=8.0, uniform_mix=0.01, max_length=4)
    with pytest.raises(ValueError, match="bandwidth"):
        ev([[sp, sp]], ["a"], bandwidth=-1.0, uniform_mix=0.01, max_length=4)
    means, per_key = ev([[], []], ["a", "b"], bandwidth=8.0, uniform_mix=0.01, max_length=4)
    assert per_key["keys"] == ["a", "b"] and np.isnan(per_key["GOLD"]).all() and per_key["dropped"].tolist() == [0, 0]
    assert np.isnan(means["GOLD"]) and means["GOLD_count"] == 0 and means["GOLD_nan_keys"] == 2 and means["dropped"] == 0


def test_no_cpu_path(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import scanpath_kde as M
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    sp = np.array([[1.0, 1.0]])
    with pytest.raises(hip.HipError, match="no CPU path"):
        M.kde_cell_baselines([sp, sp], [0, 1], (24, 32), (3, 4), bandwidth=8.0)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M.kde_leave_out_likelihood([sp, sp], [0, 1], (24, 32), (3, 4), bandwidth=8.0, uniform_mix=0.0, leave="image")


def test_information_gain_explained_and_table_merge():
    from scanpaths_amd.utils import evaluation as E
    table = E.LikelihoodTable()
    table.add({"LL": 1.5, "LL_sum": 15.0, "LL_count": 10, "LL_nan": 0, "LL_nan_keys": 0, "IG": 0.5, "IG_sum": 5.0, "IG_count": 10,
               "IG_nan": 0, "IG_nan_keys": 0, "dropped": 1})
    table.add({"GOLD": 3.0, "GOLD_sum": 24.0, "GOLD_count": 8, "GOLD_nan": 2, "GOLD_nan_keys": 0})
    table.add({"GOLD": 2.0, "GOLD_sum": 4.0, "GOLD_count": 2, "GOLD_nan": 1, "GOLD_nan_keys": 1})
    means = table.result()
    assert means["GOLD"] == 2.8 and means["GOLD_count"] == 10 and means["GOLD_nan"] == 3 and means["GOLD_nan_keys"] == 1
    assert means["LL"] == 1.5 and means["IG"] == 0.5 and means["dropped"] == 1
    res = E.information_gain_explained(means, means)
    assert res["BASE"] == 1.0 and abs(res["IG_gold"] - 1.8) <= 1e-15 and abs(res["IGE"] - 0.5 / 1.8) <= 1e-15
    assert (res["LL_count"], res["IG_count"], res["GOLD_count"]) == (10, 10, 10)
    assert E.information_gain_explained(means, {"GOLD": 3.0, "GOLD_count": 4})["IG_gold"] == 2.0      # two dicts
    res = E.information_gain_explained({"LL": 1.5, "LL_count": 3}, means)                             # no IG
    assert np.isnan(res["BASE"]) and np.isnan(res["IG_gold"]) and np.isnan(res["IGE"]) and res["IG_count"] == 0
    res = E.information_gain_explained(means, {})                                                     # no gold standard
    assert res["BASE"] == 1.0 and np.isnan(res["IG_gold"]) and np.isnan(res["IGE"]) and res["GOLD_count"] == 0
    for gold in (1.0, 0.5, float("-inf")):                                                           # a ceiling not above the baseline
        res = E.information_gain_explained(means, {"GOLD": gold, "GOLD_count": 1})
        assert np.isnan(res["IGE"]) and res["IG_gold"] == gold - 1.0
