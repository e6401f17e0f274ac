"""The bootstrap without a device: the draw rule, the restatement tests/bootstrap_ref.py against numpy on what does not
depend on a summation order, every refusal of bootstrap_ratio before a device or the library is touched, the pure-numpy helpers, the
key matching of the keyed functions (run through the restatement), the entry points of the library, and the method itself: a bootstrap
standard error next to the textbook one, unclustered and clustered."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import abi
import bootstrap_ref as R
from sampling_ref import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def M():
    from scanpaths_amd.utils.evaltools import bootstrap
    return bootstrap


@pytest.fixture
def no_device(monkeypatch):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch

    def fail(*a, **k):
        raise AssertionError("validation must come first")

    monkeypatch.setattr(_batch, "device", fail)
    monkeypatch.setattr(hip, "lib", fail)


@pytest.fixture
def on_host(monkeypatch):
    """the keyed functions with the restatement in place of the device call"""
    def ratio(num, den, clusters=None, contrasts=None, *, replicates, seed, quantiles=(0.025, 0.975), return_replicates=False):
        res = R.bootstrap(num, den, clusters, contrasts, replicates=replicates, seed=seed, quantiles=quantiles)
        if not return_replicates:
            del res["replicates"]
        return res

    monkeypatch.setattr(M(), "bootstrap_ratio", ratio)


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 64, 65])
def test_draws_lie_in_range_and_follow_the_stated_rule(C):
    seed = 0x1234_5678_9ABC_DEF0
    idx = R.draws(7, C, seed)
    assert idx.shape == (7, C) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < C
    for b in (0, 3, 6):
        for j in sorted({0, min(1, C - 1), C // 2, C - 1}):
            words = philox4x32_10((b, j >> 2, 0, 1), (seed & 0xFFFFFFFF, seed >> 32))
            assert idx[b, j] == (int(words[j & 3]) * C) >> 32
    assert (R.draws(2, C, seed, b0=5) == idx[5:7]).all()
    if C > 1:
        assert (R.draws(7, C, seed + 1) != idx).any()


def test_draws_at_the_cluster_limit():
    C = M().MAX_CLUSTERS
    assert C == 1 << 24
    idx = R.draws(1, C, 99)
    assert idx.shape == (1, C) and idx.min() >= 0 and idx.max() < C
    assert len(np.unique(idx)) > C // 2                               # 1 - 1/e of the clusters are expected


def test_the_stream_differs_from_the_samplers():
    """the fourth counter word: (b, 0, 0, 1) here, (row, 0, 0, 0) in the sampler"""
    ours = philox4x32_10((np.arange(8), 0, 0, 1), (5, 0))
    theirs = philox4x32_10((np.arange(8), 0, 0, 0), (5, 0))
    assert all((a != b).all() for a, b in zip(ours, theirs))


# ---- the restatement against numpy ------------------------------------------------------------------------------------------------------------
def test_point_estimate_is_the_nanmean_over_keys():
    """values on a dyadic grid, so that every order of adding them is exact and the comparison needs no tolerance"""
    g = np.random.default_rng(3)
    value = g.integers(-4096, 4096, (150, 3)) / 64.0
    value[g.random((150, 3)) < 0.2] = NAN
    value[:, 2] = NAN
    value[0, 2] = 1.5
    per_key = {"keys": list(range(150)), "a": value[:, 0], "b": value[:, 1], "c": value[:, 2]}
    num, den, keys = M().table_columns(per_key, ["a", "b", "c"])
    labels = g.integers(0, 40, 150)
    labels[:40] = np.arange(40)
    N, D = R.cluster_sums(num, den, labels, 40)
    est = R.estimate(N, D, [(0, -1, -1, -1), (1, -1, -1, -1), (2, -1, -1, -1), (0, 1, -1, -1)])
    want = np.nanmean(value, 0)
    assert (est[:3] == want).all() and est[3] == want[0] - want[1]
    own = R.bootstrap(num, den, None, None, replicates=2, seed=1)["estimate"]          # every key its own cluster
    assert (own == want).all()


def test_ordered_sums_stay_within_the_bound_of_the_exact_ones():
    g = np.random.default_rng(4)
    T = g.uniform(0.5, 2.0, (130, 2))
    idx = R.draws(5, 130, 8)
    got, exact = R.replicate_sums(T, idx), R.replicate_sums_fsum(T, idx)
    assert (np.abs(got - exact) <= 2 * 131 * 2.0 ** -53 * exact).all()
    assert (R.replicate_sums(T[:3], np.array([[2, 0, 1]])) == (T[2] + T[1]) + T[0]).all()      # lanes 0, 1, 2: (l0 + l2) + (l1 + 0)


def test_summary_of_the_restatement():
    v = np.array([[3.0, NAN, -1.0, 0.0, 0.0, 2.0, NAN, -INF, INF, 5.0],
                  [NAN] * 10,
                  [1.0] * 10,
                  [4.0, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN]])
    q = np.array([0.0, 0.025, 0.5, 0.975, 1.0])
    s = R.summary(v, q)
    assert s["n_valid"].tolist() == [8, 0, 10, 1] and s["n_le0"].tolist() == [4, 0, 0, 0] and s["n_ge0"].tolist() == [6, 0, 10, 1]
    assert s["quantiles"][0].tolist() == [-INF, -INF, 0.0, INF, INF]                # ranks 0, 0, 3, 7, 7 of -inf -1 0 0 2 3 5 inf
    assert np.isnan(s["quantiles"][1]).all() and np.isnan(s["mean"][1]) and np.isnan(s["se"][1])
    assert np.isnan(s["mean"][0]) and np.isnan(s["se"][0])                          # -inf + inf
    assert s["mean"][2] == 1.0 and s["se"][2] == 0.0 and (s["quantiles"][2] == 1.0).all()
    assert s["mean"][3] == 4.0 and np.isnan(s["se"][3]) and (s["quantiles"][3] == 4.0).all()
    w = np.random.default_rng(5).normal(3.0, 1.0, (1, 777))
    t = R.summary(w, q)
    assert t["mean"][0] == pytest.approx(w.mean(), rel=1e-13) and t["se"][0] == pytest.approx(w.std(ddof=1), rel=1e-13)
    assert [R.quantile_rank(x, 777) for x in q] == [0, 19, 388, 757, 776]
    assert (t["quantiles"][0] == np.sort(w[0])[[0, 19, 388, 757, 776]]).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_a_device_or_the_library(no_device):
    ratio = M().bootstrap_ratio
    num, den = np.ones((6, 3)), np.ones((6, 3))
    kw = dict(replicates=10, seed=1)
    p = inspect.signature(ratio).parameters
    assert list(p) == ["num", "den", "clusters", "contrasts", "replicates", "seed", "quantiles", "return_replicates"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("replicates", "seed", "quantiles", "return_replicates"))
    assert p["replicates"].default is inspect.Parameter.empty and p["seed"].default is inspect.Parameter.empty
    with pytest.raises(TypeError):
        ratio(num, den)
    with pytest.raises(ValueError, match="equal shapes"):
        ratio(num, np.ones((6, 2)), **kw)
    with pytest.raises(ValueError, match="equal shapes"):
        ratio(num, np.ones((5, 3)), **kw)
    with pytest.raises(ValueError, match=r"\[G, M\]"):
        ratio(np.ones((2, 2, 2)), np.ones((2, 2, 2)), **kw)
    with pytest.raises(ValueError, match="G = 0"):
        ratio(np.ones((0, 3)), np.ones((0, 3)), **kw)
    with pytest.raises(ValueError, match="one cluster label per key"):
        ratio(num, den, [0, 1, 2], **kw)
    for bad in ([0, 1, 2, 0.5, 1, 2], [0, 1, 2, NAN, 1, 2], ["a"] * 6, [True] * 6):
        with pytest.raises(ValueError, match="integers"):
            ratio(num, den, bad, **kw)
    with pytest.raises(ValueError, match="negative"):
        ratio(num, den, [0, 1, 2, -1, 1, 2], **kw)
    with pytest.raises(ValueError, match="dense"):
        ratio(num, den, [0, 1, 3, 0, 1, 3], **kw)
    with pytest.raises(ValueError, match="2\\^24"):
        ratio(num, den, [0, 1, 2, 3, 4, 1 << 24], **kw)
    for bad in ([(3, -1, -1, -1)], [(-1, -1, -1, -1)], [(0, -2, -1, -1)], [(0, 1, 3, -1)], [(0, 1, 2, 7)]):
        with pytest.raises(ValueError, match="contrast index out of range"):
            ratio(num, den, None, bad, **kw)
    with pytest.raises(ValueError, match="integers"):
        ratio(num, den, None, [(0.5, -1, -1, -1)], **kw)
    for bad in ([(0, 1, 2)], [0, 1, 2, 3], np.zeros((0, 4), int)):
        with pytest.raises(ValueError, match=r"\[S, 4\]"):
            ratio(num, den, None, bad, **kw)
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="replicates"):
            ratio(num, den, replicates=bad, seed=1)
    for bad in (-1, 1 << 64, 0.5, None):
        with pytest.raises(ValueError, match="seed"):
            ratio(num, den, replicates=10, seed=bad)
    for bad in ((-0.1, 0.5), (0.5, 1.0000001), (NAN,)):
        with pytest.raises(ValueError, match="quantiles"):
            ratio(num, den, quantiles=bad, **kw)
    with pytest.raises(AssertionError, match="validation must come first"):          # a good call gets as far as the device
        ratio(num, den, [0, 0, 1, 1, 2, 2], [(0, 1, 2, -1)], quantiles=(0, 1), **kw)


def test_every_key_its_own_cluster_is_held_to_the_limit_too(no_device, monkeypatch):
    monkeypatch.setattr(M(), "MAX_CLUSTERS", 5)
    with pytest.raises(ValueError, match="exceed the limit"):
        M().bootstrap_ratio(np.ones(6), np.ones(6), replicates=1, seed=0)


def test_no_cpu_path(monkeypatch):
    import torch
    from scanpaths_amd import hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="HIP device only"):
        M().bootstrap_ratio(np.ones(4), np.ones(4), replicates=3, seed=0)


# ---- the pure-numpy helpers -----------------------------------------------------------------------------------------------------------------
def test_table_columns_on_two_batches_that_share_a_key():
    t1 = {"keys": ["q1", "q2"], "SS": np.array([0.5, NAN]), "FED": np.array([3.0, 4.0]), "dropped": np.array([0, 1])}
    t2 = {"keys": ["q2", "q3"], "SS": np.array([0.25, 1.0]), "FED": np.array([NAN, -INF])}
    num, den, keys = M().table_columns([t1, t2], ["SS", "FED"])
    assert keys == ["q1", "q2", "q2", "q3"]
    assert num.tolist() == [[0.5, 3.0], [0.0, 4.0], [0.25, 0.0], [1.0, -INF]]
    assert den.tolist() == [[1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]]
    assert M().key_clusters(keys).tolist() == [0, 1, 1, 2]                            # the shared key: two rows of one cluster
    assert M().key_clusters(keys, {"q1": "im1", "q2": "im1", "q3": "im2"}).tolist() == [0, 0, 0, 1]
    assert M().key_clusters(keys, ["x", "y", "x", "y"]).tolist() == [0, 1, 0, 1]
    one = M().table_columns(t1, ["FED"])
    assert one[0].shape == (2, 1) and one[2] == ["q1", "q2"]
    with pytest.raises(ValueError, match="no image for key 'q3'"):
        M().key_clusters(keys, {"q1": 0, "q2": 0})
    with pytest.raises(ValueError, match="one cluster key per key"):
        M().key_clusters(keys, [0, 1])
    with pytest.raises(ValueError, match="no entry 'DTW'"):
        M().table_columns(t1, ["DTW"])
    with pytest.raises(ValueError, match="one value per key"):
        M().table_columns({"keys": [1, 2], "SS": np.zeros(3)}, ["SS"])
    with pytest.raises(ValueError, match="at least one"):
        M().table_columns([], ["SS"])


def test_column_chunks_keep_a_contrasts_columns_together():
    limit = 4
    con = np.array([(0, -1, -1, -1), (1, -1, -1, -1), (2, -1, -1, -1), (3, 0, -1, -1), (4, 3, 0, 1), (5, -1, 5, -1), (0, 5, -1, -1)])
    chunks = M().column_chunks(con, limit)
    assert [c.tolist() for c, _ in chunks] == [[0, 1, 2, 3], [4, 3, 0, 1], [5, 0]]
    assert [k.tolist() for _, k in chunks] == [[[0, -1, -1, -1], [1, -1, -1, -1], [2, -1, -1, -1], [3, 0, -1, -1]], [[0, 1, 2, 3]],
                                               [[0, -1, 0, -1], [1, 0, -1, -1]]]
    rebuilt = [[cols[m] if m >= 0 else -1 for m in row] for cols, local in chunks for row in local]
    assert rebuilt == con.tolist()
    wide = M().column_chunks(M()._check_contrasts(None, 2 * M().MAX_COLUMNS + 1))
    assert [len(c) for c, _ in wide] == [M().MAX_COLUMNS, M().MAX_COLUMNS, 1]


# ---- the keyed functions, through the restatement -----------------------------------------------------------------------------------------
def _tables():
    g = np.random.default_rng(11)
    keys = [f"q{i}" for i in range(12)]
    a = {"keys": keys, "DTW": g.normal(5.0, 1.0, 12), "REC": g.uniform(0, 1, 12), "dropped": np.zeros(12, np.int64)}
    order = g.permutation(12)
    b = {"keys": [keys[i] for i in order], "DTW": (a["DTW"] + g.normal(0.3, 0.1, 12))[order], "REC": a["REC"][order].copy()}
    a["REC"][2] = NAN
    b["DTW"][0] = NAN                                                                 # key order[0]
    images = {k: i // 3 for i, k in enumerate(keys)}
    return a, b, order, images


def test_bootstrap_evaluation_on_the_host(on_host):
    from scanpaths_amd.utils import evaluation as E
    a, _, _, images = _tables()
    res = E.bootstrap_evaluation(a, cluster_keys=images, replicates=200, seed=2)
    assert list(res) == ["DTW", "REC"]                                                # every float64 [G] entry, not the int64 one
    for name in res:
        assert res[name]["estimate"] == float(a[name][~np.isnan(a[name])].mean())
        assert res[name]["lo"] <= res[name]["estimate"] <= res[name]["hi"] and res[name]["se"] > 0 and res[name]["n_valid"] == 200
    aligned = E.bootstrap_evaluation(a, names=["DTW"], cluster_keys=[images[k] for k in a["keys"]], replicates=200, seed=2)
    assert aligned["DTW"] == res["DTW"]
    want = R.bootstrap(*M().table_columns(a, ["DTW"])[:2], M().key_clusters(a["keys"], images), replicates=200, seed=2,
                       quantiles=(0.025, 0.975))
    assert res["DTW"]["se"] == want["se"][0] and (res["DTW"]["lo"], res["DTW"]["hi"]) == tuple(want["quantiles"][0])
    assert E._level_quantiles(0.95) == (0.025, 0.975) and E._level_quantiles(0.9) == (0.05, 0.95)
    for bad in (0, 1, 1.5, None, True):
        with pytest.raises(ValueError, match="level"):
            E.bootstrap_evaluation(a, replicates=10, seed=1, level=bad)
    with pytest.raises(TypeError):
        E.bootstrap_evaluation(a, seed=1)


def test_bootstrap_comparison_matches_by_key(on_host):
    from scanpaths_amd.utils import evaluation as E
    a, b, order, images = _tables()
    res = E.bootstrap_comparison(a, b, cluster_keys=images, replicates=300, seed=4)
    assert list(res) == ["DTW", "REC"]
    inv = np.argsort(order)                                                           # b's row of a's key i
    assert (E._match_rows(a["keys"], b["keys"]) == inv).all()
    for name in res:
        va, vb = a[name], b[name][inv]
        both = ~np.isnan(va) & ~np.isnan(vb)
        assert both.sum() == 11
        assert res[name]["a"] == pytest.approx(va[both].mean(), rel=1e-14) and res[name]["b"] == pytest.approx(vb[both].mean(), rel=1e-14)
        assert res[name]["difference"] == res[name]["a"] - res[name]["b"]
    assert res["DTW"]["hi"] < 0 and res["DTW"]["p"] == 2 / 301                         # b is worse by 0.3 +- 0.1 on every key
    assert res["REC"]["difference"] == 0 and res["REC"]["lo"] == res["REC"]["hi"] == 0 and res["REC"]["p"] == 1.0
    same = E.bootstrap_comparison(a, a, cluster_keys=images, replicates=50, seed=4)
    assert all(v["difference"] == 0 and v["lo"] == v["hi"] == 0 and v["se"] == 0 and v["p"] == 1.0 for v in same.values())
    # the ValueError names the missing key, whichever side lacks it
    short = {k: v[:-1] for k, v in b.items()}
    with pytest.raises(ValueError, match=repr(b["keys"][-1])):
        E.bootstrap_comparison(a, short, replicates=10, seed=1)
    with pytest.raises(ValueError, match=repr(b["keys"][-1])):
        E.bootstrap_comparison(short, a, replicates=10, seed=1)
    twice = [a, {k: v[:1] for k, v in a.items()}]                                     # two batches that share q0: b holds it once
    with pytest.raises(ValueError, match="'q0'"):
        E.bootstrap_comparison(twice, b, replicates=10, seed=1)


def test_missing_key_is_refused_without_a_device(no_device):
    from scanpaths_amd.utils import evaluation as E
    a, b, _, _ = _tables()
    with pytest.raises(ValueError, match="missing"):
        E.bootstrap_comparison(a, {k: v[1:] for k, v in b.items()}, replicates=10, seed=1)
    with pytest.raises(ValueError, match="missing"):
        E.bootstrap_information_gain_explained({"keys": [1, 2], "LL": np.ones(2), "IG": np.ones(2)}, {"keys": [1], "GOLD": np.ones(1)},
                                               replicates=10, seed=1)


def test_information_gain_explained_is_one_contrast(on_host):
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(13)
    keys = list(range(20))
    t = {"keys": keys, "LL": g.normal(1.0, 0.2, 20), "IG": g.normal(0.4, 0.1, 20)}
    gold = {"keys": keys[::-1], "GOLD": g.normal(1.6, 0.2, 20)}
    t["IG"][3] = NAN
    t["LL"][5] = t["IG"][5] = -INF                                                     # BASE would be NaN: the key leaves
    gold["GOLD"][0] = NAN                                                              # key 19
    ok = np.ones(20, bool)
    ok[[3, 5, 19]] = False
    res = E.bootstrap_information_gain_explained(t, gold, replicates=400, seed=6)
    means = {"LL": t["LL"][ok].mean(), "IG": t["IG"][ok].mean()}
    want = E.information_gain_explained(means, {"GOLD": gold["GOLD"][::-1][ok].mean()})
    assert list(res) == ["IGE", "IG_gold", "BASE"]
    assert res["BASE"]["estimate"] == pytest.approx((t["LL"][ok] - t["IG"][ok]).mean(), rel=1e-13)
    for name in res:
        assert res[name]["estimate"] == pytest.approx(want[name], rel=1e-12)
        assert res[name]["lo"] < res[name]["estimate"] < res[name]["hi"] and res[name]["n_valid"] == 400


# ---- the library --------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_points_and_the_limit():
    lib = abi.assert_declared({"sp_boot_max_columns": ("int", 0), "sp_boot_cluster_sums": ("int", 10), "sp_boot_resample": ("int", 12),
                               "sp_boot_summarise": ("int", 12)})
    assert lib.sp_boot_max_columns() == M().MAX_COLUMNS
    assert "scanboot.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()
    # the launchers refuse before any launch (no device needed): null pointers and shapes outside their domain
    one = ctypes.c_void_p(8)
    assert lib.sp_boot_cluster_sums(None, one, one, one, 1, 1, 1, one, one, None) == -2
    assert lib.sp_boot_cluster_sums(one, one, one, one, 0, 1, 1, one, one, None) == -1
    assert lib.sp_boot_cluster_sums(one, one, one, one, 1, (1 << 24) + 1, 1, one, one, None) == -1
    assert lib.sp_boot_resample(one, one, 1, 1, 1, None, 1, 1, 0, one, one, None) == -2
    for C, Mc, ld, S, B in ((0, 1, 1, 1, 1), ((1 << 24) + 1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, M().MAX_COLUMNS + 1, 64, 1, 1),
                            (1, 2, 1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0)):
        assert lib.sp_boot_resample(one, one, C, Mc, ld, one, S, B, 0, one, one, None) == -1, (C, Mc, ld, S, B)
    assert lib.sp_boot_summarise(None, 1, 1, one, 1, one, one, one, one, one, one, None) == -2
    assert lib.sp_boot_summarise(one, 1, 1, None, 1, one, one, one, one, one, one, None) == -2
    for S, B, Q in ((0, 1, 1), (1, 0, 1), (1, 1, -1)):
        assert lib.sp_boot_summarise(one, S, B, one, Q, one, one, one, one, one, one, None) == -1


# ---- the method itself, on the restatement ----------------------------------------------------------------------------------------------
def test_the_standard_error_is_the_textbook_one_and_clustering_widens_it():
    """G = C = 400 iid standard normal values, B = 2000: the bootstrap se of the mean lies within 20 % of std(ddof=1) / sqrt(400) -- the
    relative spread of a bootstrap se is about sqrt(1 / (2 B) + 1 / (2 G)) = 4 %, so 20 % is five of those.  With the 400 keys in 40
    clusters of 10 and a shared per-cluster offset of variance 1 the clustered se exceeds the unclustered one by a factor above 2
    (expected: about sqrt(1 + 10) = 3.3)."""
    g = np.random.default_rng(2024)
    v = g.normal(size=400)
    plain = R.bootstrap(v, np.ones(400), None, None, replicates=2000, seed=7)
    textbook = v.std(ddof=1) / math.sqrt(400)
    print("se", plain["se"][0], "textbook", textbook)
    assert abs(plain["se"][0] / textbook - 1.0) < 0.2
    assert plain["n_valid"][0] == 2000 and plain["quantiles"][0, 0] < plain["estimate"][0] < plain["quantiles"][0, 1]
    labels = np.repeat(np.arange(40), 10)
    w = v + g.normal(size=40)[labels]
    loose = R.bootstrap(w, np.ones(400), None, None, replicates=2000, seed=7)
    tight = R.bootstrap(w, np.ones(400), labels, None, replicates=2000, seed=7)
    print("clustered se", tight["se"][0], "unclustered", loose["se"][0])
    assert tight["se"][0] > 2.0 * loose["se"][0]
