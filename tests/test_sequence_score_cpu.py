"""CPU-only checks of the sequence-score layer: the four entry points are declared, bound and exported with equal
signatures and refuse bad arguments before any launch; the Python checker (tests/seqscore_ref.py) holds the known answers and the
properties of the definitions, its quick variant equals its plain-loop variant bit for bit, and it agrees with sklearn's MeanShift where
that is installed; every argument refusal of the Python layer is raised before a device or the library is touched."""
import inspect

import numpy as np
import pytest

import abi
import seqscore_ref as R

NEW = {"sp_meanshift_max_points": ("int", 0), "sp_meanshift": ("int", 12), "sp_scan_cluster_strings": ("int", 11),
       "sp_scan_sequence": ("int", 9)}
# four-fold symmetric: four clusters of three points, equal in k; (10, 10) and (10, -10) tie in x (y decides), two seeds of a cluster
# reach the bit-identical centre (the seed index decides their order)
SYMMETRIC = np.array([[s * 10.0 + a, t * 10.0 + b] for s in (1, -1) for t in (1, -1) for a, b in ((0, 0), (1, 0), (-1, 0))])


def test_new_entry_points_are_declared_bound_and_exported():
    from scanpaths_amd.utils.evaltools import sequence_score as S
    lib = abi.assert_declared(NEW, prefixes=("sp_meanshift_", "sp_scan_sequence_", "sp_scan_cluster_strings_"))
    assert lib.sp_meanshift_max_points() == S.MAX_POINTS >= 1024
    assert lib.sp_scan_max_fixations() == S.MAX_FIXATIONS == R.MAX_FIXATIONS == 64


def test_launchers_refuse_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too"""
    lib = abi.raw_lib()
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")
    MS, CS, SQ = lib.sp_meanshift, lib.sp_scan_cluster_strings, lib.sp_scan_sequence
    ms = [p, 2, p, p, 1, 25.0, 300, p, p, None, None, None]         # weight and labels may be NULL
    for k in (0, 2, 3, 7, 8):
        assert MS(*[None if i == k else a for i, a in enumerate(ms)]) == -2, k
    for k, bad in ((4, 0), (4, -1), (1, 1), (5, 0.0), (5, -1.0), (5, nan), (5, inf), (6, 0), (6, -3)):
        assert MS(*[bad if i == k else a for i, a in enumerate(ms)]) == -1, (k, bad)
    cs = [p, 2, p, p, p, 1, p, p, p, p, None]
    for k in (0, 2, 3, 4, 6, 7, 8, 9):
        assert CS(*[None if i == k else a for i, a in enumerate(cs)]) == -2, k
    for k, bad in ((5, 0), (5, -2), (1, 1), (1, 0)):
        assert CS(*[bad if i == k else a for i, a in enumerate(cs)]) == -1, (k, bad)
    sq = [p, p, p, p, 1, 0.0, p, p, None]
    for k in (0, 1, 2, 3):
        assert SQ(*[None if i == k else a for i, a in enumerate(sq)]) == -2, k
    assert SQ(p, p, p, p, 1, 0.0, None, None, None) == -2           # both outputs NULL
    for k, bad in ((4, 0), (4, -1), (5, 0.5), (5, nan), (5, -inf), (5, inf)):
        assert SQ(*[bad if i == k else a for i, a in enumerate(sq)]) == -1, (k, bad)


def _ms(points, h, **kw):
    c, w, lab = R.meanshift_loops(np.array(points, dtype=np.float64), h, **kw)
    return c.tolist(), w.tolist(), lab.tolist()


def test_checker_known_answers_mean_shift():
    assert _ms([(10, 10)] * 3, 5) == ([[10.0, 10.0]], [3], [0, 0, 0])
    assert _ms([(0, 0), (5, 0)], 5) == ([[2.5, 0.0]], [2], [0, 0])                           # 25 <= 25: the <= boundary
    assert _ms([(0, 0), (11, 0)], 5) == ([[11.0, 0.0], [0.0, 0.0]], [1, 1], [1, 0])          # equal k: x descending
    assert _ms([(0, 0), (3, 0), (6, 0), (9, 0)], 3) == ([[6.0, 0.0], [1.5, 0.0]], [3, 2], [1, 1, 0, 0])
    c, w, lab = _ms(SYMMETRIC, 5)
    assert c == [[10.0, 10.0], [10.0, -10.0], [-10.0, 10.0], [-10.0, -10.0]] and w == [3, 3, 3, 3]
    assert lab == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert _ms(np.zeros((0, 2)), 5) == ([], [], [])
    # a point exactly between two centres takes the lower cluster
    assert R.labels_of([(5.0, 0.0), (5.5, 0.0), (4.5, 0.0)], [(10.0, 0.0), (0.0, 0.0)]).tolist() == [0, 0, 1]
    assert R.labels_of([(5.0, 0.0)], np.zeros((0, 2))).tolist() == [-1]
    # only columns 0 and 1 are read
    g = np.random.default_rng(3)
    P = g.integers(0, 60, (40, 2)).astype(np.float64)
    a, b = R.meanshift_loops(P, 12.0), R.meanshift_loops(np.concatenate([P, g.uniform(-9, 9, (40, 3))], 1), 12.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_checker_known_answers_strings():
    assert R.sequence_score([0, 1, 2, 3], [0, 2, 3]) == 0.75 and R.fixation_edit_distance([0, 1, 2, 3], [0, 2, 3]) == 1.0
    a = [3, 1, 4, 1, 5, 9, 2, 6]
    assert R.sequence_score(a, a) == 1.0 and R.fixation_edit_distance(a, a) == 0.0
    assert R.fixation_edit_distance(a, []) == len(a) == R.fixation_edit_distance([], a)
    assert R.sequence_score(a, []) == 0.0 and R.sequence_score(a, [], gap=-0.5) == -0.5
    assert np.isnan(R.sequence_score([], [])) and R.fixation_edit_distance([], []) == 0.0
    assert R.sequence_score([0, 1], [1, 0], gap=-1.0) == 0.0                                 # two mismatches beat gap + match + gap
    assert R.sequence_score([0, 1, 2], [2], gap=-0.5) == (1.0 - 0.5 - 0.5) / 3.0
    assert np.isnan(R.sequence_score([0, -1], [0])) and np.isnan(R.fixation_edit_distance([0], [0, -1]))
    assert np.isnan(R.sequence_score([0] * 65, [0])) and np.isnan(R.fixation_edit_distance([0], [0] * 65))


def test_checker_properties_on_seeded_string_pairs():
    g = np.random.default_rng(17)
    for t in range(2000):
        n, m = int(g.integers(0, 65)), int(g.integers(0, 65))
        sym = (1, 2, 12)[t % 3]
        a, b = g.integers(0, sym, n).tolist(), g.integers(0, sym, m).tolist()
        ss, fed = R.sequence_score(a, b), R.fixation_edit_distance(a, b)
        assert np.array_equal(ss, R.sequence_score(b, a), equal_nan=True) and fed == R.fixation_edit_distance(b, a), (t, a, b)
        if n == m == 0:
            assert np.isnan(ss) and fed == 0.0
            continue
        L = max(n, m)
        assert 0.0 <= ss <= 1.0
        common = R.lcs(a, b)
        assert R.nw_table_end(a, b, 0.0) == common and ss == common / L, (t, ss, common)     # gap 0: exact in integers
        assert L - common <= fed <= n + m - 2 * common, (t, fed, common, n, m)
        gapped = R.sequence_score(a, b, gap=-0.1 * (1 + t % 4))
        assert gapped <= ss and gapped == R.sequence_score(b, a, gap=-0.1 * (1 + t % 4))


def _group(g, grid, npts=None):
    """2-7 object centres in a 320 x 240 frame, 8-119 points around them with sigma 12, the first fifth uniform, clipped"""
    k = int(g.integers(2, 8))
    n = int(g.integers(8, 120)) if npts is None else npts
    obj = g.uniform((0, 0), (320, 240), (k, 2))
    P = obj[g.integers(0, k, n)] + g.normal(0, 12, (n, 2))
    P[:n // 5] = g.uniform((0, 0), (320, 240), (n // 5, 2))
    P = np.clip(P, (0, 0), (320, 240))
    return np.round(P) if grid else P


def test_quick_checker_equals_the_plain_loops_bit_for_bit():
    g = np.random.default_rng(5)
    for t in range(24):
        P = _group(g, grid=t % 2 == 0, npts=(1, 2, 3, 17, 40, 90)[t % 6])
        for h, it in ((10.0, 300), (25.0, 300), (50.0, 2), (25.0, 1)):
            a, b = R.meanshift_loops(P, h, it), R.meanshift(P, h, it)
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)), (t, h, it)
    a, b = R.meanshift_loops(SYMMETRIC, 5.0), R.meanshift(SYMMETRIC, 5.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_checker_against_sklearn_meanshift():
    """All 360 groups: the same K, labels_ and predict of fresh points, centres within 1e-9 px (sklearn sums its means in another
    order: a few ulp of 320 over at most ~120 values, 1.14e-13 measured; 1e-9 leaves four orders).  The two documented differences
     would show as a differing K or label; none does on this seed."""
    cluster = pytest.importorskip("sklearn.cluster")
    g = np.random.default_rng(0)
    worst = 0.0
    for grid in (True, False):
        for h in (10.0, 25.0, 50.0):
            for t in range(60):
                P = _group(g, grid)
                fresh = g.uniform((0, 0), (320, 240), (40, 2))
                ms = cluster.MeanShift(bandwidth=h, bin_seeding=False, cluster_all=True).fit(P)
                c, w, lab = R.meanshift(P, h)
                assert len(c) == len(ms.cluster_centers_), (grid, h, t)
                assert np.array_equal(lab, ms.labels_), (grid, h, t)
                assert np.array_equal(R.predict(fresh, c), ms.predict(fresh)), (grid, h, t)
                err = float(np.abs(c - ms.cluster_centers_).max())
                worst = max(worst, err)
                assert err <= 1e-9, (grid, h, t, err)
    print(f"worst centre difference {worst:.3g}")
    P = np.random.default_rng(1).integers(0, 101, (80, 2)).astype(np.float64)
    for it in (1, 2, 5):
        ms = cluster.MeanShift(bandwidth=15.0, bin_seeding=False, cluster_all=True, max_iter=it).fit(P)
        c, w, lab = R.meanshift(P, 15.0, it)
        assert np.array_equal(c, ms.cluster_centers_) and np.array_equal(lab, ms.labels_), it


def test_public_surface():
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import sequence_score as S
    assert S.METRICS == R.METRICS == ("SS", "FED")
    p = inspect.signature(S.meanshift_clusters).parameters
    assert list(p) == ["groups_of_points", "bandwidth", "max_iter"] and p["max_iter"].default == 300
    assert p["bandwidth"].kind is inspect.Parameter.KEYWORD_ONLY and p["bandwidth"].default is inspect.Parameter.empty
    assert list(inspect.signature(S.cluster_strings).parameters) == ["scanpaths", "groups", "clusters"]
    p = inspect.signature(S.sequence_scores_pairs).parameters
    assert list(p) == ["strings", "pairs", "metrics", "gap"] and p["metrics"].default == ("SS", "FED") and p["gap"].default == 0.0
    p = inspect.signature(S.sequence_score).parameters
    assert list(p) == ["human", "simulated", "centres", "gap"] and p["gap"].default == 0.0
    assert list(inspect.signature(S.fixation_edit_distance).parameters) == ["human", "simulated", "centres"]
    p = inspect.signature(E.sequence_score_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "bandwidth", "metrics", "gap", "max_iter",
                       "cluster_keys"]
    q = inspect.signature(E.sequence_score_human_evaluation).parameters
    assert list(q) == ["gt_fix_vectors", "gt_keys", "bandwidth", "metrics", "gap", "max_iter", "cluster_keys"]
    for sig in (p, q):
        assert sig["bandwidth"].kind is inspect.Parameter.KEYWORD_ONLY and sig["bandwidth"].default is inspect.Parameter.empty
        assert sig["metrics"].default == ("SS", "FED") and sig["gap"].default == 0.0 and sig["max_iter"].default == 300
        assert sig["cluster_keys"].default is None


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import sequence_score as S

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(S, "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    P = np.array([[0.0, 0.0], [3.0, 0.0], [40.0, 5.0]])
    cen = np.array([[1.5, 0.0], [40.0, 5.0]])
    long = np.zeros((S.MAX_FIXATIONS + 1, 2))
    with pytest.raises(TypeError):
        S.meanshift_clusters([P])                                                     # no default bandwidth
    for h in (0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth"):
            S.meanshift_clusters([P], bandwidth=h)
        with pytest.raises(ValueError, match="bandwidth"):
            E.sequence_score_evaluation([P], [P], ["a"], ["a"], bandwidth=h)
        with pytest.raises(ValueError, match="bandwidth"):
            E.sequence_score_human_evaluation([P, P], ["a", "a"], bandwidth=h)
    for it in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_iter"):
            S.meanshift_clusters([P], bandwidth=5.0, max_iter=it)
        with pytest.raises(ValueError, match="max_iter"):
            E.sequence_score_evaluation([P], [P], ["a"], ["a"], bandwidth=5.0, max_iter=it)
    with pytest.raises(ValueError, match="kernel limit"):
        S.meanshift_clusters([P, np.zeros((S.MAX_POINTS + 1, 2))], bandwidth=5.0)
    with pytest.raises(ValueError, match="columns"):
        S.meanshift_clusters([P, np.zeros((3, 3))], bandwidth=5.0)
    with pytest.raises(ValueError, match="kernel limit"):
        S.cluster_strings([P, long], [0, 0], [cen])
    for bad in ([0, 1], [-1, 0]):
        with pytest.raises(ValueError, match="out of range"):
            S.cluster_strings([P, P], bad, [cen])
    with pytest.raises(ValueError, match="one group per scanpath"):
        S.cluster_strings([P, P], [0], [cen])
    strings, pairs = [[0, 1, 2], [0, 2]], [(0, 1)]
    with pytest.raises(ValueError, match="unknown"):
        S.sequence_scores_pairs(strings, pairs, metrics=("SS", "DTW"))
    with pytest.raises(ValueError, match="repeated"):
        S.sequence_scores_pairs(strings, pairs, metrics=("FED", "FED"))
    with pytest.raises(ValueError, match="no sequence metric"):
        S.sequence_scores_pairs(strings, pairs, metrics=())
    for gap in (0.5, float("nan"), float("-inf"), float("inf")):
        with pytest.raises(ValueError, match="gap"):
            S.sequence_scores_pairs(strings, pairs, gap=gap)
        with pytest.raises(ValueError, match="gap"):
            S.sequence_score(P, P, cen, gap=gap)
        with pytest.raises(ValueError, match="gap"):
            E.sequence_score_evaluation([P], [P], ["a"], ["a"], bandwidth=5.0, gap=gap)
    with pytest.raises(ValueError, match="kernel limit"):
        S.sequence_scores_pairs([[0] * 65, [0]], pairs)
    with pytest.raises(ValueError, match="labels"):
        S.sequence_scores_pairs([[0, -2], [0]], pairs)
    for bad in ([(0, 2)], [(-1, 0)], [(0, 1), (5, 0)]):
        with pytest.raises(ValueError, match="out of range"):
            S.sequence_scores_pairs(strings, bad)
    with pytest.raises(ValueError, match="kernel limit"):
        S.sequence_score(long, P, cen)
    with pytest.raises(ValueError, match="kernel limit"):
        S.fixation_edit_distance(P, long, cen)
    # empty input: empty output, no device
    assert S.meanshift_clusters([], bandwidth=5.0) == []
    (c, w, lab), = S.meanshift_clusters([np.zeros((0, 2))], bandwidth=5.0)
    assert c.shape == (0, 2) and w.shape == (0,) and lab.shape == (0,) and lab.dtype == np.int32
    assert S.cluster_strings([], [], [cen]) == []
    res = S.sequence_scores_pairs(strings, [])
    assert list(res) == ["SS", "FED"] and all(v.shape == (0,) and v.dtype == np.float64 for v in res.values())
    # evaluation level
    fv = [P, P[::-1].copy()]
    with pytest.raises(TypeError):
        E.sequence_score_evaluation(fv, fv, ["a", "b"], ["a", "b"])                  # bandwidth is required
    with pytest.raises(TypeError):
        E.sequence_score_human_evaluation(fv, ["a", "a"])
    with pytest.raises(ValueError, match="not among gt_keys"):
        E.sequence_score_evaluation(fv, fv, ["a", "b"], ["a", "c"], bandwidth=5.0)
    with pytest.raises(ValueError, match="one key per"):
        E.sequence_score_evaluation(fv, fv, ["a"], ["a", "a"], bandwidth=5.0)
    with pytest.raises(ValueError, match="one key per"):
        E.sequence_score_human_evaluation(fv, ["a"], bandwidth=5.0)
    with pytest.raises(ValueError, match="unknown"):
        E.sequence_score_evaluation(fv, fv, ["a", "b"], ["a", "b"], bandwidth=5.0, metrics=("SED",))
    with pytest.raises(ValueError, match="two images"):
        E.sequence_score_evaluation(fv, fv, ["a", "a"], ["a", "a"], bandwidth=5.0, cluster_keys=["x", "y"])
    with pytest.raises(ValueError, match="kernel limit"):
        E.sequence_score_evaluation([long, P], [P], ["a", "a"], ["a"], bandwidth=5.0)
    big = [np.zeros((64, 2))] * 17                                                   # 1088 fixations on one key
    with pytest.raises(ValueError, match="kernel limit"):
        E.sequence_score_human_evaluation(big, ["a"] * 17, bandwidth=5.0)
    means, per_key = E.sequence_score_evaluation(fv, [], ["a", "b"], [], bandwidth=5.0)      # no pairs: NaN tables, no device
    assert per_key["keys"] == ["a", "b"] and all(np.isnan(per_key[m]).all() for m in ("SS", "FED", "SS_best", "FED_best"))
    assert means["SS_nan"] == 2 and np.isnan(means["FED_best"])
