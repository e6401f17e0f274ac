"""CPU-only checks of the DTW / Frechet / Hausdorff / Eyenalysis / cross-recurrence layer: the two entry points are declared, bound and
exported with equal signatures; the Python checker (tests/scanpath_dist_ref.py) holds the sanity values, inequalities and symmetries of
DESIGN.md §16; the public signatures are the documented ones; every argument refusal of the Python layer is raised before a device or
the library is touched."""
import inspect

import numpy as np
import pytest

import abi
import scanpath_dist_ref as R

NEW = {"sp_scan_distances": ("int", 12), "sp_scan_recurrence": ("int", 11)}


def test_new_entry_points_are_declared_bound_and_exported():
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    lib = abi.assert_declared(NEW, prefixes=("sp_scan_distances_", "sp_scan_recurrence_"))
    assert lib.sp_scan_max_fixations() == M.MAX_FIXATIONS == 64      # the limit the Python layer refuses by, without the library


def test_launchers_refuse_bad_arguments_without_a_device():
    """the argument checks of the two launchers come before the launch: SP_ENULL (-2) / SP_EINVAL (-1) on a machine without a GPU too"""
    lib = abi.raw_lib()
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    D, Rc = lib.sp_scan_distances, lib.sp_scan_recurrence
    assert D(p, 2, p, p, p, 1, 1.0, None, None, None, None, None) == -2            # all four outputs NULL
    for k in range(4):
        args = [p, 2, p, p, p, 1, 1.0, p, None, None, None, None]
        args[(0, 2, 3, 4)[k]] = None
        assert D(*args) == -2
    assert D(p, 2, p, p, p, 0, 1.0, p, None, None, None, None) == -1               # npairs < 1
    assert D(p, 1, p, p, p, 1, 1.0, p, None, None, None, None) == -1               # ncol < 2
    for md in (0.0, -1.0, float("nan")):
        assert D(p, 2, p, p, p, 1, md, p, None, None, None, None) == -1
        assert Rc(p, 2, p, p, p, 1, md, 1.0, 2, p, None) == -1
    assert Rc(p, 2, p, p, p, 1, 1.0, 1.0, 2, None, None) == -2
    assert Rc(None, 2, p, p, p, 1, 1.0, 1.0, 2, p, None) == -2
    assert Rc(p, 2, p, p, p, 0, 1.0, 1.0, 2, p, None) == -1
    assert Rc(p, 1, p, p, p, 1, 1.0, 1.0, 2, p, None) == -1
    for rad in (0.0, -2.0, float("nan")):
        assert Rc(p, 2, p, p, p, 1, 1.0, rad, 2, p, None) == -1
    assert Rc(p, 2, p, p, p, 1, 1.0, 1.0, 1, p, None) == -1                        # min_line < 2


SQUARE = np.array([[100.0, 100.0], [200.0, 100.0], [200.0, 200.0], [100.0, 200.0]])


def _all(P, Q, radius, L=2, max_dim=1.0):
    return (R.dtw(P, Q, max_dim), R.frechet(P, Q, max_dim), R.hausdorff(P, Q, max_dim), R.eyenalysis(P, Q, max_dim)) + \
        R.cross_recurrence(P, Q, radius, L, max_dim)


def test_checker_sanity_values():
    assert _all(SQUARE, SQUARE, 10.0) == (0.0, 0.0, 0.0, 0.0, 25.0, 100.0, 0.0, 0.0)
    rec, det, _, _ = R.cross_recurrence(SQUARE, SQUARE[::-1], 10.0)
    assert (rec, det) == (25.0, 0.0)
    assert R.cross_recurrence(SQUARE, np.repeat(SQUARE[:1], 4, 0), 10.0) == (25.0, 0.0, 50.0, 50.0)
    # by hand: P on a line, Q the same line shifted up by 3 with one more point
    P = np.array([[0.0, 0.0], [4.0, 0.0], [8.0, 0.0]])
    Q = np.array([[0.0, 3.0], [4.0, 3.0], [8.0, 3.0], [12.0, 3.0]])
    assert R.dtw(P, Q) == 3.0 + 3.0 + 3.0 + 5.0 and R.frechet(P, Q) == 5.0 and R.hausdorff(P, Q) == 5.0
    assert R.eyenalysis(P, Q) == (3.0 * 3 + (3.0 * 3 + 5.0)) / 4.0
    # recurrence by hand, N = 3 (the fourth fixation of Q is cut): d <= 5 on the main and the two neighbouring diagonals
    assert R.cross_recurrence(P, Q, 5.0) == (100.0 * 7 / 9, 100.0, 100.0 * 14 / 14, 0.0)
    assert R.cross_recurrence(P, Q, 5.0, min_line=3) == (100.0 * 7 / 9, 100.0 * 3 / 7, 100.0 * 6 / 14, 0.0)
    # NaN rules
    E = np.zeros((0, 2))
    assert all(np.isnan(v) for v in _all(E, SQUARE, 10.0) + _all(SQUARE, E, 10.0) + _all(E, E, 10.0))
    rec, det, lam, corm = R.cross_recurrence(SQUARE, SQUARE + 50.0, 10.0)          # R = 0
    assert rec == 0.0 and np.isnan(det) and np.isnan(lam) and np.isnan(corm)
    rec, det, lam, corm = R.cross_recurrence(SQUARE[:1], SQUARE, 10.0)             # N = 1
    assert (rec, det, lam) == (100.0, 0.0, 0.0) and np.isnan(corm)
    # only columns 0 and 1 are read; max_dim divides the coordinates, so the radius shrinks with it
    P3 = np.concatenate([P, np.full((3, 2), 7.0)], 1)
    Q3 = np.concatenate([Q, np.full((4, 2), -1.0)], 1)
    assert _all(P3, Q3, 5.0) == _all(P, Q, 5.0)
    assert R.dtw(P, Q, 4.0) == 14.0 / 4.0 and R.cross_recurrence(P, Q, 5.0 / 4.0, 2, 4.0) == R.cross_recurrence(P, Q, 5.0)


def test_checker_inequalities_and_symmetries_on_grid_pairs():
    """2000 seeded pairs on an 8-pixel grid, lengths 1..19.  DTW, Frechet, Hausdorff and REC are exactly symmetric under swapping P and Q
    and CORM changes its sign exactly.  Eyenalysis is symmetric only up to the rounding of its sum: the definition adds the n row
    minima first and then the m column minima term by term, the swapped pair adds the same n + m non-negative terms with the two groups
    in the other order, and floating-point addition is not associative (624 of these 2000 pairs differ, by at most 4 ulp).  Each of
    the n + m - 1 additions of either order errs by at most 2^-53 of a partial sum that does not exceed the total, and the division adds
    half an ulp, so the two values differ by less than 2 (n + m) ulp: that is what is asserted for it."""
    g = np.random.Generator(np.random.PCG64(16))
    for t in range(2000):
        n, m = int(g.integers(1, 20)), int(g.integers(1, 20))
        P, Q = g.integers(0, 8, (n, 2)) * 8.0, g.integers(0, 8, (m, 2)) * 8.0
        radius, L = (8.0, 12.0, 16.0)[t % 3], 2 + t % 2
        a, b = _all(P, Q, radius, L), _all(Q, P, radius, L)
        assert a[2] <= a[1] <= a[0], (t, a)                                        # Hausdorff <= Frechet <= DTW
        assert a[:3] == b[:3] and a[4] == b[4], (t, a, b)                          # exactly symmetric, REC included
        assert abs(a[3] - b[3]) <= 2 * (n + m) * np.spacing(max(a[3], b[3])), (t, a[3], b[3])
        assert np.array_equal(a[7], -b[7], equal_nan=True), (t, a, b)              # CORM changes sign exactly
        assert np.array_equal(a[5:7], b[5:7], equal_nan=True)                      # so do DET and LAM stay (the matrix is transposed)
        assert 0.0 <= a[4] <= 100.0 and (np.isnan(a[5]) or (0.0 <= a[5] <= 100.0 and 0.0 <= a[6] <= 100.0))
        assert np.isnan(a[7]) == (min(n, m) == 1 or a[4] == 0.0) and (np.isnan(a[7]) or -100.0 <= a[7] <= 100.0)


def test_public_surface():
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    assert M.SCANPATH_DISTANCES == ("DTW", "Frechet", "Hausdorff", "Eyenalysis", "REC", "DET", "LAM", "CORM")
    assert R.DISTANCES + R.RECURRENCE == M.SCANPATH_DISTANCES
    p = inspect.signature(M.scanpath_distances_pairs).parameters
    assert list(p) == ["scanpaths", "pairs", "metrics", "max_dim", "radius", "min_line"]
    assert p["max_dim"].default == 1.0 and p["radius"].default is None and p["min_line"].default == 2
    for fn in (M.DTW, M.frechet_distance, M.hausdorff_distance, M.eyenalysis_distance):
        assert list(inspect.signature(fn).parameters) == ["human_scanpath", "simulated_scanpath"]
    p = inspect.signature(M.cross_recurrence).parameters
    assert list(p) == ["human_scanpath", "simulated_scanpath", "radius", "min_line"]
    assert p["radius"].kind is inspect.Parameter.KEYWORD_ONLY and p["radius"].default is inspect.Parameter.empty
    assert p["min_line"].kind is inspect.Parameter.KEYWORD_ONLY and p["min_line"].default == 2
    p = inspect.signature(E.scanpath_distance_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "metrics", "max_dim", "radius", "min_line"]
    q = inspect.signature(E.scanpath_distance_human_evaluation).parameters
    assert list(q) == ["gt_fix_vectors", "gt_keys", "metrics", "max_dim", "radius", "min_line"]
    for sig in (p, q):
        assert sig["metrics"].kind is inspect.Parameter.KEYWORD_ONLY and sig["metrics"].default is inspect.Parameter.empty
        assert sig["max_dim"].default == 1.0 and sig["radius"].default is None and sig["min_line"].default == 2


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M

    def no_lib():
        raise AssertionError("validation must come first")

    def no_device():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M, "_device", no_device)
    monkeypatch.setattr(hip, "lib", no_lib)
    a, b = SQUARE, SQUARE[::-1].copy()
    paths, pairs = [a, b], [(0, 1)]
    with pytest.raises(ValueError, match="unknown"):
        M.scanpath_distances_pairs(paths, pairs, metrics=("DTW", "Levenshtein"))
    with pytest.raises(ValueError, match="repeated"):
        M.scanpath_distances_pairs(paths, pairs, metrics=("DTW", "DTW"))
    with pytest.raises(TypeError, match="radius"):
        M.scanpath_distances_pairs(paths, pairs, metrics=("DTW", "REC"))
    with pytest.raises(TypeError):
        M.cross_recurrence(a, b)
    with pytest.raises(TypeError, match="radius"):
        M.cross_recurrence(a, b, radius=None)
    for rad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            M.scanpath_distances_pairs(paths, pairs, metrics=("REC",), radius=rad)
        with pytest.raises(ValueError, match="radius"):
            M.cross_recurrence(a, b, radius=rad)
    for md in (0.0, -320.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dim"):
            M.scanpath_distances_pairs(paths, pairs, metrics=("DTW",), max_dim=md)
    for ml in (1, 0, -3, 2.5):
        with pytest.raises(ValueError, match="min_line"):
            M.scanpath_distances_pairs(paths, pairs, metrics=("DET",), radius=10.0, min_line=ml)
        with pytest.raises(ValueError, match="min_line"):
            M.cross_recurrence(a, b, radius=10.0, min_line=ml)
    long = np.zeros((M.MAX_FIXATIONS + 1, 2))
    with pytest.raises(ValueError, match="kernel limit"):
        M.scanpath_distances_pairs([a, long], pairs)
    with pytest.raises(ValueError, match="kernel limit"):
        M.DTW(long, a)
    for bad in ([(0, 2)], [(-1, 0)], [(0, 1), (5, 0)]):
        with pytest.raises(ValueError, match="out of range"):
            M.scanpath_distances_pairs(paths, bad)
    with pytest.raises(ValueError, match="columns"):
        M.scanpath_distances_pairs([a, np.zeros((3, 3))], pairs)
    # an empty pair list: empty arrays, no device
    res = M.scanpath_distances_pairs(paths, [], metrics=M.SCANPATH_DISTANCES, radius=10.0)
    assert list(res) == list(M.SCANPATH_DISTANCES) and all(v.shape == (0,) and v.dtype == np.float64 for v in res.values())
    # evaluation level
    fv = [a, b]
    with pytest.raises(TypeError):
        E.scanpath_distance_evaluation(fv, fv, ["a", "b"], ["a", "b"])                       # metrics is required
    with pytest.raises(ValueError, match="not among gt_keys"):
        E.scanpath_distance_evaluation(fv, fv, ["a", "b"], ["a", "c"], metrics=("DTW",))
    with pytest.raises(ValueError, match="one key per"):
        E.scanpath_distance_evaluation(fv, fv, ["a"], ["a", "a"], metrics=("DTW",))
    with pytest.raises(TypeError, match="radius"):
        E.scanpath_distance_evaluation(fv, fv, ["a", "b"], ["a", "b"], metrics=("LAM",))
    with pytest.raises(ValueError, match="unknown"):
        E.scanpath_distance_evaluation(fv, fv, ["a", "b"], ["a", "b"], metrics=("SED",))
    with pytest.raises(TypeError, match="radius"):
        E.scanpath_distance_human_evaluation(fv, ["a", "a"], metrics=("CORM",))
    with pytest.raises(ValueError, match="one key per"):
        E.scanpath_distance_human_evaluation(fv, ["a"], metrics=("DTW",))
    with pytest.raises(ValueError, match="min_line"):
        E.scanpath_distance_human_evaluation(fv, ["a", "a"], metrics=("DET",), radius=5.0, min_line=1)
