"""The bootstrap on the device against the ordered restatement tests/bootstrap_ref.py: replicates, point estimate and
summary bit for bit (NaN equal to NaN) over the Philox word and block boundaries, the lane tail, a second stride, the
four-waves-per-block tail and the column chunks; the sums within the textbook bound of the exact (fsum) ones; non-finite values;
every contrast shape; ties, quantile ranks and zero counts of the summary; the keyed functions on real scorer output; determinism and
what is copied back."""
import numpy as np
import pytest
import torch

import bootstrap_ref as R

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
Q5 = (0.0, 0.025, 0.5, 0.975, 1.0)
FIELDS = ("estimate", "mean", "se", "quantiles", "n_valid", "n_le0", "n_ge0")


def M():
    from scanpaths_amd.utils.evaltools import bootstrap
    return bootstrap


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1)) if got.dtype.kind == "f" \
        else np.flatnonzero((got != want).reshape(-1))
    assert not len(bad), (what, len(bad), bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def both(num, den, clusters=None, contrasts=None, *, replicates, seed, quantiles=Q5):
    """the device's result and the restatement's, compared in every field; returns the device's with the replicates on the host"""
    got = M().bootstrap_ratio(num, den, clusters, contrasts, replicates=replicates, seed=seed, quantiles=quantiles, return_replicates=True)
    want = R.bootstrap(num, den, clusters, contrasts, replicates=replicates, seed=seed, quantiles=quantiles)
    assert isinstance(got["replicates"], torch.Tensor) and got["replicates"].is_cuda and got["replicates"].dtype == torch.float64
    got["replicates"] = got["replicates"].cpu().numpy()
    for k in ("replicates",) + FIELDS:
        same(got[k], want[k], k)
    return got


def uneven_labels(C, g):
    """2 C + 6 keys in C clusters: cluster 0 holds more than half of the keys, cluster min(1, C - 1) three, the others are singletons;
    shuffled, so that a cluster's keys are not neighbours"""
    labels = np.concatenate([np.arange(C), np.zeros(C + 4, np.int64), np.full(2, min(1, C - 1))])
    return labels[g.permutation(len(labels))]


def table(G, Mc, g):
    return g.normal(1.0, 2.0, (G, Mc)), g.uniform(0.5, 1.5, (G, Mc))


# ---- replicates, point estimate and summary against the ordered restatement ------------------------------------------------------------
SHAPES = [(C, 5, 3) for C in (1, 3, 4, 5, 63, 64, 65, 130)] + [(65, B, 2) for B in (1, 3, 4, 257)]


@pytest.mark.parametrize("C,B,Mc", SHAPES)
def test_replicates_estimate_and_summary_are_the_restatements(C, B, Mc):
    g = np.random.default_rng(1000 * C + B)
    labels = uneven_labels(C, g)
    num, den = table(len(labels), Mc, g)
    con = [(m, -1, -1, -1) for m in range(Mc)] + [(0, Mc - 1, -1, -1), (0, -1, Mc - 1, 0), (Mc - 1, 0, 0, -1)]
    got = both(num, den, labels, con, replicates=B, seed=(C << 32) + B)
    assert got["replicates"].shape == (Mc + 3, B) and got["n_valid"].dtype == np.int32


def test_every_key_its_own_cluster():
    g = np.random.default_rng(2)
    num, den = table(70, 2, g)
    got = both(num, den, replicates=9, seed=5)
    same(got["estimate"], R.estimate(num, den, [(0, -1, -1, -1), (1, -1, -1, -1)]), "estimate without cluster sums")


@pytest.mark.parametrize("Mc", [1, 32, 33, 65])
def test_column_chunks_give_the_bits_of_the_columns_launched_alone(Mc):
    assert M().MAX_COLUMNS == 32
    g = np.random.default_rng(Mc)
    labels = uneven_labels(5, g)
    num, den = table(len(labels), Mc, g)
    got = both(num, den, labels, replicates=4, seed=77)
    for m in sorted({0, Mc // 2, Mc - 1}):
        alone = M().bootstrap_ratio(num[:, m], den[:, m], labels, replicates=4, seed=77, quantiles=Q5, return_replicates=True)
        same(alone["replicates"].cpu().numpy()[0], got["replicates"][m], f"column {m} alone")
        for k in FIELDS:
            same(alone[k][0], got[k][m], k)


def test_a_contrast_takes_its_columns_along_into_its_chunk():
    g = np.random.default_rng(8)
    labels = uneven_labels(5, g)
    num, den = table(len(labels), 65, g)
    con = [(m, -1, -1, -1) for m in range(31)] + [(64, 2, 40, 31), (3, 64, -1, -1), (50, -1, -1, -1)]     # the 32nd contrast needs 3 new columns
    assert [len(c) for c, _ in M().column_chunks(np.array(con))] == [31, 6]
    got = both(num, den, labels, con, replicates=5, seed=3)
    cols = [64, 2, 40, 31]
    alone = M().bootstrap_ratio(num[:, cols], den[:, cols], labels, [(0, 1, 2, 3)], replicates=5, seed=3, return_replicates=True)
    same(alone["replicates"].cpu().numpy()[0], got["replicates"][31], "the moved contrast alone")


def test_sums_lie_within_the_textbook_bound_of_the_exact_ones():
    """strictly positive num and den: every replicate within 2 (n + 1) 2^-53 relative of fsum(num) / fsum(den) over the drawn keys, n =
    the number of terms added = C draws plus the largest cluster's members.  Worst observed on an MI355X: 6.0e-16 against the bound 5.9e-14."""
    g = np.random.default_rng(21)
    C, B = 130, 257
    labels = uneven_labels(C, g)
    num, den = g.uniform(0.1, 10.0, (len(labels), 2)), g.uniform(0.5, 1.5, (len(labels), 2))
    got = both(num, den, labels, replicates=B, seed=9)
    exact = R.exact_ratios(num, den, labels, R.draws(B, C, 9))
    n = C + int(np.bincount(labels).max())
    err = np.abs(got["replicates"].T - exact) / exact
    print("worst relative error", err.max(), "bound", 2 * (n + 1) * 2.0 ** -53)
    assert err.max() <= 2 * (n + 1) * 2.0 ** -53
    N, D = R.cluster_sums(num, den, labels, C)                                    # the same bound against the restatement's fsum form
    loose = R.resample(N, D, [(0, -1, -1, -1), (1, -1, -1, -1)], B, 9, sums=R.replicate_sums_fsum)
    assert (np.abs(got["replicates"] - loose) <= 2 * (n + 1) * 2.0 ** -53 * loose).all()


# ---- non-finite values ----------------------------------------------------------------------------------------------------------------------
def test_a_nan_key_in_one_column_only():
    g = np.random.default_rng(31)
    labels = uneven_labels(5, g)
    value = g.normal(size=(len(labels), 2))
    value[3, 0] = NAN
    num, den, _ = M().table_columns({"keys": list(range(len(labels))), "a": value[:, 0], "b": value[:, 1]}, ["a", "b"])
    got = both(num, den, labels, replicates=40, seed=1)                           # the nanmean rule: the key leaves column a only
    assert got["n_valid"].tolist() == [40, 40] and got["estimate"][1] == pytest.approx(value[:, 1].mean(), rel=1e-13)
    assert got["estimate"][0] == pytest.approx(np.nanmean(value[:, 0]), rel=1e-13)
    raw = value.copy()                                                            # a NaN that reaches the sums poisons its column only
    got = both(raw, np.ones_like(raw), labels, replicates=40, seed=1)
    assert 0 < got["n_valid"][0] < 40 and got["n_valid"][1] == 40 and np.isnan(got["estimate"][0])


def test_a_column_that_is_nan_throughout():
    g = np.random.default_rng(32)
    labels = uneven_labels(4, g)
    num, den = table(len(labels), 2, g)
    num[:, 1] = den[:, 1] = 0.0                                                   # a table entry that is NaN for every key: 0 / 0
    got = both(num, den, labels, replicates=7, seed=2)
    assert got["n_valid"].tolist() == [7, 0] and got["n_le0"][1] == got["n_ge0"][1] == 0
    assert np.isnan(got["se"][1]) and np.isnan(got["mean"][1]) and np.isnan(got["quantiles"][1]).all() and np.isnan(got["estimate"][1])


def test_two_clusters_one_of_them_empty_of_values():
    """C = 2, cluster 1 all NaN (num = den = 0): a replicate that draws it twice is 0 / 0 -- about a quarter of them"""
    num, den, labels = np.array([1.5, 2.5, 0.0, 0.0]), np.array([1.0, 1.0, 0.0, 0.0]), [0, 0, 1, 1]
    want = R.bootstrap(num, den, labels, replicates=64, seed=13)
    assert 64 - want["n_valid"][0] >= 1 and want["n_valid"][0] >= 2
    got = both(num, den, labels, replicates=64, seed=13)
    assert got["n_valid"][0] == want["n_valid"][0] == 47 and got["se"][0] == 0.0 and (got["quantiles"][0] == 2.0).all()


def test_infinite_values_are_scores():
    g = np.random.default_rng(33)
    labels = uneven_labels(5, g)
    num, den = table(len(labels), 2, g)
    den[:] = 1.0
    i, j = int(np.flatnonzero(labels == 2)[0]), int(np.flatnonzero(labels == 3)[0])
    num[i, 0] = -INF
    num[i, 1], num[j, 1] = INF, -INF                                               # +inf and -inf in one column: a replicate with both is NaN
    got = both(num, den, labels, replicates=60, seed=4)
    r = got["replicates"]
    drew = (R.draws(60, 5, 4) == 2).any(1)
    assert drew.any() and not drew.all() and (r[0][drew] == -INF).all() and np.isfinite(r[0][~drew]).all()
    assert got["quantiles"][0, 0] == -INF and np.isfinite(got["quantiles"][0, -1]) and got["mean"][0] == -INF and np.isnan(got["se"][0])
    assert got["n_valid"][0] == 60 and got["estimate"][0] == -INF
    assert np.isnan(r[1]).any() and (r[1] == INF).any() and (r[1] == -INF).any() and np.isnan(got["estimate"][1])


# ---- contrasts ------------------------------------------------------------------------------------------------------------------------------
def test_every_contrast_shape():
    g = np.random.default_rng(41)
    labels = uneven_labels(7, g)
    num, den = table(len(labels), 4, g)
    con = [(2, -1, -1, -1), (0, 1, -1, -1), (0, -1, 2, 3), (0, 1, 1, -1), (3, 3, -1, -1), (1, 0, 3, 2)]
    got = both(num, den, labels, con, replicates=33, seed=6)
    r = got["replicates"]
    plain = both(num, den, labels, replicates=33, seed=6)["replicates"]
    same(r[0], plain[2], "plain")
    same(r[1], plain[0] - plain[1], "difference")
    same(r[2], plain[0] / (plain[2] - plain[3]), "ratio of differences")
    same(r[3], (plain[0] - plain[1]) / plain[1], "relative improvement")
    assert (r[4] == 0).all()


def test_a_denominator_that_is_zero_in_every_replicate():
    """C = 1: every replicate is the data, so R[1] - R[1] = 0 and the contrast is R[0] / 0 = +-inf, or 0 / 0 = NaN"""
    num, den = np.array([[2.0, 1.0, -3.0], [1.0, 5.0, -1.0]]), np.ones((2, 3))
    con = [(0, -1, 1, 1), (2, -1, 1, 1), (0, 0, 1, 1)]
    got = both(num, den, [0, 0], con, replicates=6, seed=1)
    assert (got["replicates"][0] == INF).all() and (got["replicates"][1] == -INF).all() and np.isnan(got["replicates"][2]).all()
    assert got["estimate"][0] == INF and got["n_valid"].tolist() == [6, 6, 0] and (got["quantiles"][1] == -INF).all()


def test_the_entry_points_guard_what_the_host_never_sends():
    """at the C ABI: a run of keys outside [0, G) reads nothing and gives NaN sums; a contrast index that is not a column of the launch
    gives NaN and addresses no memory"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    dev = torch.device("cuda", torch.cuda.current_device())
    L = hip.lib()
    num = np.arange(1.0, 9.0).reshape(4, 2)
    con = np.array([(0, -1, -1, -1), (2, -1, -1, -1), (0, 5, -1, -1), (1, -1, 0, -3), (-1, -1, -1, -1), (1, 0, -1, -1)], dtype=np.int32)
    buf, at = _batch.upload({"num": num, "den": np.ones((4, 2)), "starts": np.array([0, 2, 3, -1], np.int64),
                             "counts": np.array([2, 1, 2, 1], np.int32), "contrast": con}, dev)
    out = _batch.Out({"N": (np.float64, 8), "D": (np.float64, 8), "stat": (np.float64, 6 * 3), "estimate": (np.float64, 6)}, dev)
    hip.check(L.sp_boot_cluster_sums(at["num"], at["den"], at["starts"], at["counts"], 4, 4, 2, out.ptr("N"), out.ptr("D"), hip.stream()), "sums")
    hip.check(L.sp_boot_resample(out.ptr("N"), out.ptr("D"), 2, 2, 2, at["contrast"], 6, 3, 1, out.ptr("stat"), out.ptr("estimate"),
                                 hip.stream()), "resample")                       # the two good clusters only
    res = out.host()
    same(res["N"].reshape(4, 2), np.array([[4.0, 6.0], [5.0, 6.0], [NAN, NAN], [NAN, NAN]]), "N")     # 3 + 2 > G; start -1
    same(res["D"].reshape(4, 2), np.array([[2.0, 2.0], [1.0, 1.0], [NAN, NAN], [NAN, NAN]]), "D")
    same(res["estimate"], np.array([3.0, NAN, NAN, NAN, NAN, 1.0]), "estimate")   # (4 + 5) / 3 and (6 + 6) / 3 - 3
    stat = res["stat"].reshape(6, 3)
    assert np.isnan(stat[1:5]).all() and not np.isnan(stat[[0, 5]]).any()


# ---- the summary ----------------------------------------------------------------------------------------------------------------------------
def test_ties_quantile_ranks_one_replicate_and_zero_counts():
    g = np.random.default_rng(51)
    num, den = table(6, 2, g)
    tied = both(num, den, [0] * 6, replicates=300, seed=2)                        # C = 1: every replicate equals the estimate
    for m in range(2):
        assert (tied["replicates"][m] == tied["estimate"][m]).all() and (tied["quantiles"][m] == tied["estimate"][m]).all()
        assert tied["n_valid"][m] == 300 and tied["se"][m] == 0.0
    labels = uneven_labels(9, g)
    num, den = table(len(labels), 3, g)
    num[:, 2] = 0.0                                                                # replicates that are exactly 0
    got = both(num, den, labels, [(0, -1, -1, -1), (2, -1, -1, -1), (1, 1, -1, -1)], replicates=261, seed=3)
    v = np.sort(got["replicates"][0])
    assert got["quantiles"][0].tolist() == v[[0, 6, 130, 254, 260]].tolist()       # ceil(q * 261) - 1
    assert got["n_le0"].tolist()[1:] == [261, 261] and got["n_ge0"].tolist()[1:] == [261, 261]
    assert got["n_le0"][0] + got["n_ge0"][0] == 261
    one = both(num, den, labels, replicates=1, seed=3)
    assert np.isnan(one["se"]).all() and (one["mean"] == one["replicates"][:, 0]).all() and (one["quantiles"] == one["mean"][:, None]).all()


# ---- the keyed functions on real scorer output --------------------------------------------------------------------------------------------
def _scored(seed):
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(seed)
    keys = ["im0/q0", "im0/q1", "im1/q0", "im1/q1", "im2/q0", "im2/q1"]
    gt = [g.uniform(0, 300, (int(g.integers(3, 9)), 2)) for _ in keys for _ in range(2)]
    gt_keys = [k for k in keys for _ in range(2)]
    pr = [g.uniform(0, 300, (int(g.integers(3, 9)), 2)) for _ in keys for _ in range(2)]
    means, per_key = E.scanpath_distance_evaluation(gt, pr, gt_keys, gt_keys, metrics=("DTW", "Frechet", "Eyenalysis"))
    return means, per_key, {k: k.split("/")[0] for k in keys}


def test_keyed_functions_on_a_scorers_own_table():
    from scanpaths_amd.utils import evaluation as E
    means, t, images = _scored(1)
    assert len(t["keys"]) == 6
    res = E.bootstrap_evaluation(t, cluster_keys=images, replicates=200, seed=5)
    names = [k for k in t if k != "keys"]
    assert list(res) == names and len(names) >= 3
    for name in names:
        assert res[name]["estimate"] == means[name], name
        assert res[name]["lo"] <= res[name]["estimate"] <= res[name]["hi"] and res[name]["se"] > 0 and res[name]["n_valid"] == 200
    aligned = E.bootstrap_evaluation(t, names=names[:1], cluster_keys=[images[k] for k in t["keys"]], replicates=200, seed=5)
    assert aligned[names[0]] == res[names[0]]
    twin = E.bootstrap_comparison(t, t, cluster_keys=images, replicates=100, seed=5)
    for name in names:
        assert twin[name]["difference"] == 0 and twin[name]["lo"] == twin[name]["hi"] == 0 and twin[name]["p"] == 1.0
        assert twin[name]["a"] == twin[name]["b"] and twin[name]["n_valid"] == 100
    _, u, _ = _scored(2)
    u = {k: (v[::-1] if k == "keys" else v[::-1].copy()) for k, v in u.items()}       # the same keys in another order
    cmp = E.bootstrap_comparison(t, u, names=["DTW"], cluster_keys=images, replicates=100, seed=5)
    num = np.stack([t["DTW"], u["DTW"][::-1]], 1)
    labels = M().key_clusters(t["keys"], images)
    assert labels.tolist() == [0, 0, 1, 1, 2, 2]
    hand = M().bootstrap_ratio(num, np.ones_like(num), labels, [(0, 1, -1, -1)], replicates=100, seed=5)
    assert cmp["DTW"]["difference"] == hand["estimate"][0] and cmp["DTW"]["se"] == hand["se"][0]
    assert (cmp["DTW"]["lo"], cmp["DTW"]["hi"]) == tuple(hand["quantiles"][0])
    tail = min(int(hand["n_le0"][0]), int(hand["n_ge0"][0]))
    assert cmp["DTW"]["p"] == min(1.0, 2.0 * (tail + 1) / 101)
    with pytest.raises(ValueError, match="im2/q1"):
        E.bootstrap_comparison(t, {k: v[1:] for k, v in u.items()}, replicates=10, seed=1)


def test_information_gain_explained_on_a_hand_built_table():
    from scanpaths_amd.utils import evaluation as E
    keys = list(range(8))
    t = {"keys": keys, "LL": np.array([1.0, 1.25, 0.75, 1.5, 1.0, 0.5, 1.25, 0.75]), "IG": np.array([0.5, 0.25, 0.5, 0.75, 0.25, 0.5, 0.5, 0.25])}
    gold = {"keys": keys, "GOLD": np.array([1.5, 2.0, 1.25, 1.75, 1.5, 1.0, 2.0, 1.5])}
    res = E.bootstrap_information_gain_explained(t, gold, cluster_keys=[0, 0, 1, 1, 2, 2, 3, 3], replicates=150, seed=8)
    want = E.information_gain_explained({"LL": t["LL"].mean(), "IG": t["IG"].mean()}, {"GOLD": gold["GOLD"].mean()})
    for name in ("IGE", "IG_gold", "BASE"):                                         # dyadic values: the means are exact in any order
        assert res[name]["estimate"] == want[name], name
        assert res[name]["lo"] <= res[name]["estimate"] <= res[name]["hi"] and res[name]["n_valid"] == 150


# ---- determinism and copies ---------------------------------------------------------------------------------------------------------------
def test_the_seed_decides_and_only_the_summary_is_copied_back(monkeypatch):
    from scanpaths_amd.utils.evaltools import _batch
    g = np.random.default_rng(61)
    labels = uneven_labels(20, g)
    num, den = table(len(labels), 3, g)
    made = []

    class Recorded(_batch.Out):
        def __init__(self, sections, dev):
            made.append(dict(sections))
            super().__init__(sections, dev)

    monkeypatch.setattr(_batch, "Out", Recorded)
    run = lambda seed, **kw: M().bootstrap_ratio(num, den, labels, replicates=500, seed=seed, return_replicates=True, **kw)
    a, b, c = run(7), run(7), run(8)
    assert a["replicates"].cpu().numpy().tobytes() == b["replicates"].cpu().numpy().tobytes()
    assert all(a[k].tobytes() == b[k].tobytes() for k in FIELDS)
    assert (a["replicates"] != c["replicates"]).any().item() and (a["estimate"] == c["estimate"]).all()
    plain = M().bootstrap_ratio(num, den, labels, replicates=500, seed=7)
    assert "replicates" not in plain and sorted(plain) == sorted(FIELDS)
    assert len(made) == 4                                                          # one result buffer per call
    for sections in made:                                                          # with or without the replicates handed out
        assert sorted(sections) == sorted(FIELDS)
        assert sum(n for _, n in sections.values()) == 3 * (6 + 2)                 # S * (6 fields + Q): nothing of size S * B
