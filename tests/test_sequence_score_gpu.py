"""csrc/seqscore.hip through evaltools.sequence_score, the C entry points and the keyed evaluations, against the Python checker
tests/seqscore_ref.py -- float64 and int32, BIT FOR BIT (np.array_equal with equal_nan, no tolerance anywhere): the arithmetic is IEEE
subtract, multiply, add, divide, square root, compare and integer counting in a stated order, so a differing bit is a contraction or a
wrong summation order, not a margin.  The empty-neighbourhood exit of the mean shift (k == 0) cannot be reached from real points
 and is covered by reading the code only."""
import numpy as np
import pytest
import torch

import seqscore_ref as R

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)
LENGTHS = (0, 1, 2, 3, 5, 31, 32, 33, 63, 64)
SYMMETRIC = np.array([[s * 10.0 + a, t * 10.0 + b] for s in (1, -1) for t in (1, -1) for a, b in ((0, 0), (1, 0), (-1, 0))])
_REF = {}


def S():
    from scanpaths_amd.utils.evaltools import sequence_score
    return sequence_score


def cached(key, fn):
    """a checker result, computed once and shared read-only among the tests"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def points(g, n, grid, objects=None):
    """n points around 2-7 (or `objects`) centres of a 320 x 240 frame, sigma 12, the first fifth uniform, clipped; grid: integer pixels"""
    k = int(g.integers(2, 8)) if objects is None else objects
    obj = g.uniform((0, 0), (320, 240), (k, 2))
    P = obj[g.integers(0, k, n)] + g.normal(0, 12, (n, 2))
    P[:n // 5] = g.uniform((0, 0), (320, 240), (n // 5, 2))
    P = np.clip(P, (0, 0), (320, 240))
    return np.round(P) if grid else P


def groups_of(sizes, seed, grid, ncol=2):
    g = np.random.default_rng(seed)
    out = [points(g, n, grid) for n in sizes]
    return [np.concatenate([a, g.uniform(-1e3, 1e3, (len(a), ncol - 2))], 1) for a in out]   # further columns must not be read


def same_clusters(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("centres", "weight", "labels"), a, b):
            assert x.dtype == y.dtype and x.shape == y.shape, (what, k, name, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(x, y, equal_nan=True), (what, k, name, x, y)


def ref_clusters(tag, groups, h, max_iter=300):
    return cached(("ms", tag, h, max_iter), lambda: [R.meanshift(P, h, max_iter) for P in groups])


@pytest.mark.parametrize("h", [10.0, 25.0, 50.0])
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "offgrid"])
def test_mean_shift_group_sizes(grid, h):
    """one launch for all groups: empty, one point, below / at / above one wave and one pass of the block's seeds; integer pixels are
    tie-heavy (equal k, bit-identical centres), off-grid data is what a contracted multiply-add would change"""
    groups = groups_of(SIZES, 11 + grid, grid)
    got = S().meanshift_clusters(groups, bandwidth=h)
    want = ref_clusters(("sizes", grid), groups, h)
    print([len(c) for c, _, _ in got])
    same_clusters(got, want, f"grid={grid} h={h}")
    assert all(len(c) >= 1 for c, _, _ in got[1:]) and len(got[0][0]) == 0


@pytest.mark.parametrize("ncol", [3, 5])
def test_mean_shift_reads_two_columns(ncol):
    same_clusters(S().meanshift_clusters(groups_of(SIZES[:8], 12, True, ncol), bandwidth=25.0),
                  ref_clusters(("sizes", True), groups_of(SIZES, 12, True), 25.0)[:8], f"ncol={ncol}")


@pytest.mark.parametrize("max_iter", [1, 2, 3, 300])
def test_mean_shift_iteration_cut_off(max_iter):
    """trajectories that need more than three steps: the cut-off changes the result, and does so exactly as the definition says"""
    g = np.random.default_rng(21)
    groups = [points(g, 120, False, 3), points(g, 90, True, 2), g.uniform(0, 60, (70, 2))]
    got = S().meanshift_clusters(groups, bandwidth=25.0, max_iter=max_iter)
    same_clusters(got, ref_clusters("cut", groups, 25.0, max_iter), f"max_iter={max_iter}")
    if max_iter < 300:
        full = ref_clusters("cut", groups, 25.0, 300)
        assert any(len(a[0]) != len(b[0]) or not np.array_equal(a[0], b[0]) for a, b in zip(got, full)), "the cut-off was not reached"


def test_mean_shift_tie_breaks_alone_against_batch_and_repeat_runs():
    M = S()
    (c, w, lab), = M.meanshift_clusters([SYMMETRIC], bandwidth=5.0)
    assert c.tolist() == [[10.0, 10.0], [10.0, -10.0], [-10.0, 10.0], [-10.0, -10.0]] and w.tolist() == [3, 3, 3, 3]
    assert lab.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    (c, w, lab), = M.meanshift_clusters([[(0, 0), (5, 0)]], bandwidth=5.0)             # the <= boundary
    assert c.tolist() == [[2.5, 0.0]] and w.tolist() == [2] and lab.tolist() == [0, 0]
    (c, w, lab), = M.meanshift_clusters([[(0, 0), (3, 0), (6, 0), (9, 0)]], bandwidth=3.0)
    assert c.tolist() == [[6.0, 0.0], [1.5, 0.0]] and w.tolist() == [3, 2] and lab.tolist() == [1, 1, 0, 0]
    groups = groups_of(SIZES, 11, False) + [SYMMETRIC]
    batch = M.meanshift_clusters(groups, bandwidth=25.0)
    same_clusters(batch[:-1], ref_clusters(("sizes", False), groups[:-1], 25.0), "batch")
    for k, P in enumerate(groups):
        same_clusters(M.meanshift_clusters([P], bandwidth=25.0), [batch[k]], f"group {k} alone")
    for _ in range(2):
        same_clusters(M.meanshift_clusters(groups, bandwidth=25.0), batch, "repeat run")


def _raw_meanshift(groups, counts, h, max_iter, want_weight=True, want_labels=True, ncol=2):
    """sp_meanshift itself; counts may lie about a group (the kernel's own guard)"""
    from scanpaths_amd import hip
    L = hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = np.concatenate(groups, 0)
    pts = torch.from_numpy(rows).to(dev)
    gstart = torch.tensor(np.cumsum([0] + [len(p) for p in groups[:-1]]), dtype=torch.int64, device=dev)
    gcount = torch.tensor(counts, dtype=torch.int32, device=dev)
    centres = torch.full((len(rows), 2), 7.0, dtype=torch.float64, device=dev)
    ncentres = torch.full((len(groups),), 77, dtype=torch.int32, device=dev)
    weight = torch.full((len(rows),), 77, dtype=torch.int32, device=dev)
    labels = torch.full((len(rows),), 77, dtype=torch.int32, device=dev)
    hip.check(L.sp_meanshift(hip.ptr(pts), ncol, hip.ptr(gstart), hip.ptr(gcount), len(groups), h, max_iter, hip.ptr(centres),
                             hip.ptr(ncentres), hip.ptr(weight) if want_weight else None, hip.ptr(labels) if want_labels else None,
                             hip.stream()), "sp_meanshift")
    torch.cuda.synchronize()
    return centres.cpu().numpy(), ncentres.cpu().numpy(), weight.cpu().numpy(), labels.cpu().numpy()


def test_group_at_the_kernel_limit_and_one_beyond_it_beside_valid_groups():
    """every size of the list in one launch, the group at the limit (few clusters) and one point more included: that one gets
    ncentres -1 and labels -1, none of its points is read (they are NaN here) and its neighbours are unaffected; weight / labels NULL"""
    M = S()
    limit = M.MAX_POINTS
    g = np.random.default_rng(31)
    sizes = SIZES + (limit, limit + 1, 9)
    groups = [points(g, n, True, objects=3) for n in sizes]
    groups[-2][:] = np.nan
    start = np.cumsum([0] + [len(p) for p in groups[:-1]])
    cen, ncen, wt, lab = _raw_meanshift(groups, [len(p) for p in groups], 25.0, 300)
    want = [R.meanshift(P, 25.0) for k, P in enumerate(groups) if k != len(sizes) - 2]
    got = []
    for k, (o, n) in enumerate(zip(start, sizes)):
        if n == limit + 1:
            assert ncen[k] == -1 and (lab[o:o + n] == -1).all() and (cen[o:o + n] == 7.0).all() and (wt[o:o + n] == 77).all()
            continue
        K = int(ncen[k])
        assert 0 <= K <= n and (cen[o + K:o + n] == 7.0).all() and (wt[o + K:o + n] == 77).all()      # nothing beyond the K centres
        got.append((cen[o:o + K], wt[o:o + K], lab[o:o + n]))
    same_clusters(got, want, "limit batch")
    print("clusters of the group at the limit:", len(got[len(SIZES)][0]))
    cen2, ncen2, wt2, lab2 = _raw_meanshift(groups, [len(p) for p in groups], 25.0, 300, want_weight=False, want_labels=False)
    assert np.array_equal(cen2, cen) and np.array_equal(ncen2, ncen) and (wt2 == 77).all() and (lab2 == 77).all()
    # a negative count is refused by the kernel too; the launcher's argument checks on a live device
    _, ncen3, _, lab3 = _raw_meanshift(groups[:2] + groups[4:6], [0, -1, 63, 64], 25.0, 300)
    assert ncen3.tolist()[:2] == [0, -1] and np.array_equal(lab3[1:], np.concatenate([got[4][2], got[5][2]]))


def test_cluster_strings():
    M = S()
    cen = np.array([[10.0, 0.0], [0.0, 0.0], [10.0, 10.0], [5.0, -5.0]])
    g = np.random.default_rng(41)
    ties = np.array([[5.0, 0.0], [5.0, 5.0], [10.0, 5.0], [0.0, -5.0], [7.5, -2.5], [5.0, 5.0001], [4.9999, 0.0]])
    paths = [ties, np.zeros((0, 2)), np.array([[9.0, 9.0]]), g.integers(-4, 16, (64, 2)).astype(np.float64), g.uniform(-5, 15, (64, 2)),
             ties[::-1].copy(), g.uniform(-5, 15, (13, 2))]
    groups = [0, 0, 0, 0, 2, 1, 2]
    clusters = [cen, np.zeros((0, 2)), (cen[::-1].copy(), None, None)]               # group 1 has no centres
    got = M.cluster_strings(paths, groups, clusters)
    want = [R.labels_of(p, clusters[q][0] if isinstance(clusters[q], tuple) else clusters[q]) for p, q in zip(paths, groups)]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int32 and np.array_equal(a, b), (k, a, b)
    assert got[0].tolist() == [0, 0, 0, 1, 0, 2, 1] and got[5].tolist() == [-1] * 7 and got[1].shape == (0,)
    for ncol in (3, 5):
        wide = [np.concatenate([p, g.uniform(-9, 9, (len(p), ncol - 2))], 1) for p in paths]
        assert all(np.array_equal(a, b) for a, b in zip(M.cluster_strings(wide, groups, clusters), got))
    # under the clusters the device made itself: the labels of a group's own points
    P = points(g, 64, True)
    (c, w, lab), = M.meanshift_clusters([P], bandwidth=25.0)
    assert np.array_equal(M.cluster_strings([P], [0], [(c, w, lab)])[0], lab)


def strings_of(lengths, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, sym, n).astype(np.int32) for sym in (1, 2, 12) for n in lengths]


def same_scores(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for m in want:
        a, b = np.asarray(got[m]), np.asarray(want[m])
        assert a.dtype == np.float64 and a.shape == b.shape, (what, m, a.dtype, a.shape, b.shape)
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        print(f"{what} {m}: {int(bad.sum())} of {a.size} differ")
        assert np.array_equal(a, b, equal_nan=True), (what, m, np.flatnonzero(bad)[:8], a[bad][:8], b[bad][:8])


@pytest.mark.parametrize("gap", [0.0, -0.5, -1.0, -0.1])
def test_sequence_lengths_alphabets_and_gaps(gap):
    """all ordered pairs among lengths 0 .. 64 and alphabets of 1, 2 and 12 symbols, self-pairs included; -0.1 is inexact in binary"""
    strings = strings_of(LENGTHS, 51)
    pairs = [(a, b) for a in range(len(strings)) for b in range(len(strings))]
    got = S().sequence_scores_pairs(strings, pairs, gap=gap)
    want = {"SS": cached(("ss", gap), lambda: R.score_pairs(strings, pairs, ("SS",), gap)["SS"]),
            "FED": cached("fed", lambda: R.score_pairs(strings, pairs, ("FED",))["FED"])}
    same_scores(got, want, f"gap={gap}")
    both_empty = [k for k, (a, b) in enumerate(pairs) if len(strings[a]) == 0 and len(strings[b]) == 0]
    assert np.isnan(got["SS"][both_empty]).all() and int(np.isnan(got["SS"]).sum()) == len(both_empty) == 9
    assert not np.isnan(got["FED"]).any() and (got["FED"][both_empty] == 0.0).all()
    k = pairs.index((9, 9))                                          # 64 equal symbols against themselves
    assert got["SS"][k] == 1.0 and got["FED"][k] == 0.0


@pytest.mark.parametrize("npairs", [1, 63, 64, 65, 130])
def test_sequence_pair_counts(npairs):
    """the pairs repeat and come out of order (four pairs share a block: 1, 63 and 65 leave waves without a pair)"""
    strings = strings_of((0, 1, 2, 4, 7, 9, 12, 17), 52)
    g = np.random.default_rng(100 + npairs)
    pairs = g.integers(0, len(strings), (npairs, 2))
    pairs[npairs // 2:] = pairs[:npairs - npairs // 2][::-1]
    same_scores(S().sequence_scores_pairs(strings, pairs, gap=-0.25), R.score_pairs(strings, pairs, R.METRICS, -0.25), f"npairs={npairs}")


def test_sequence_each_output_alone_and_repeat_runs():
    M = S()
    strings = strings_of((0, 1, 3, 6, 11, 20, 33, 64), 53)
    pairs = [(a, b) for a in range(0, len(strings), 2) for b in range(len(strings))]
    both = M.sequence_scores_pairs(strings, pairs, gap=-0.1)
    same_scores(both, R.score_pairs(strings, pairs, R.METRICS, -0.1), "both")
    for m in R.METRICS:
        same_scores(M.sequence_scores_pairs(strings, pairs, metrics=(m,), gap=-0.1), {m: both[m]}, f"{m} alone")
    rev = M.sequence_scores_pairs(strings, pairs, metrics=("FED", "SS"), gap=-0.1)
    assert list(rev) == ["FED", "SS"]
    same_scores({m: rev[m] for m in R.METRICS}, both, "reversed metrics")
    for _ in range(3):
        same_scores(M.sequence_scores_pairs(strings, pairs, gap=-0.1), both, "repeat run")
    same_scores(M.sequence_scores_pairs(strings, pairs, gap=-0.0), M.sequence_scores_pairs(strings, pairs), "gap -0.0")


def test_sequence_kernel_guards_itself():
    """sp_scan_sequence directly: a pair with a label -1 and a pair with a count of 65 score NaN in both outputs; the other pairs of
    the launch are unaffected"""
    from scanpaths_amd import hip
    L = hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = np.random.default_rng(61)
    strings = [g.integers(0, 4, n).astype(np.int32) for n in (5, 65, 7, 64, 6)]
    strings[4][3] = -1
    counts = [len(s) for s in strings]
    lab = torch.from_numpy(np.concatenate(strings)).to(dev)
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    start = torch.tensor(np.cumsum([0] + counts[:-1]), dtype=torch.int64, device=dev)
    pairs = [(0, 2), (0, 1), (1, 2), (3, 3), (1, 1), (2, 0), (4, 0), (3, 1), (2, 3), (0, 4), (0, 0), (4, 4)]
    pr = torch.tensor(pairs, dtype=torch.int32, device=dev)
    n = len(pairs)
    out = torch.full((2, n), 7.0, dtype=torch.float64, device=dev)
    hip.check(L.sp_scan_sequence(hip.ptr(lab), hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, -0.5, out[0].data_ptr(), out[1].data_ptr(),
                                 hip.stream()), "sp_scan_sequence")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    bad = np.array([1 in p or 4 in p for p in pairs])
    assert np.isnan(res[:, bad]).all() and not np.isnan(res[:, ~bad]).any()
    want = R.score_pairs(strings, pairs, R.METRICS, -0.5)
    same_scores({"SS": res[0], "FED": res[1]}, want, "guarded launch")
    assert L.sp_scan_sequence(hip.ptr(lab), hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, -0.5, None, None, hip.stream()) == -2
    assert L.sp_scan_sequence(hip.ptr(lab), hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, 0.5, out[0].data_ptr(), None, hip.stream()) == -1


def _keyed_case():
    """6 keys on a 16-pixel grid: "b" has no prediction, "a" one human scanpath, "e" and "f" share an image"""
    g = np.random.default_rng(8)

    def path():
        n = int(g.integers(2, 9))
        return np.stack([g.integers(0, 8, n) * 16.0 + g.integers(-3, 4, n), g.integers(0, 6, n) * 16.0 + g.integers(-3, 4, n),
                         g.uniform(0.1, 0.5, n)], 1)

    humans = {"a": 1, "b": 2, "c": 3, "d": 4, "e": 2, "f": 3}
    preds = {"a": 2, "b": 0, "c": 3, "d": 1, "e": 2, "f": 1}
    gt_keys = [k for r in range(4) for k in "dcfbea" if r < humans[k]]
    pr_keys = [k for r in range(3) for k in "afced" if r < preds[k]]
    return [path() for _ in gt_keys], [path() for _ in pr_keys], gt_keys, pr_keys


def _nanmean(v):
    v = np.array([x for x in v if not np.isnan(x)], dtype=np.float64)
    return v.mean() if v.size else np.nan


def _by_definition(M, groups, centres_of, gap):
    """groups: key -> list of (prediction id, human scanpath, predicted scanpath); the per-pair wrappers, one pair at a time"""
    names = ["SS", "SS_best", "FED", "FED_best"]
    per_key = {nm: [] for nm in names}
    for key, trip in groups.items():
        rows = {}
        for j, h, p in trip:
            rows.setdefault(j, []).append({"SS": M.sequence_score(h, p, centres_of[key], gap=gap),
                                           "FED": M.fixation_edit_distance(h, p, centres_of[key])})
        for m, pick in (("SS", max), ("FED", min)):
            per_key[m].append(_nanmean([r[m] for rs in rows.values() for r in rs]))
            per_key[m + "_best"].append(_nanmean([pick([r[m] for r in rs if not np.isnan(r[m])], default=np.nan) for rs in rows.values()]))
    return names, {nm: np.array(v, dtype=np.float64) for nm, v in per_key.items()}


def _check_tables(means, per_key, names, want, keys):
    assert per_key["keys"] == keys and set(per_key) == set(names) | {"keys"}
    for nm in names:
        v = per_key[nm]
        print(nm, v, want[nm])
        assert np.array_equal(v, want[nm], equal_nan=True), (nm, v, want[nm])
        assert means[nm + "_nan"] == int(np.isnan(v).sum())
        assert np.array_equal(means[nm], _nanmean(v), equal_nan=True)
    assert set(means) == set(names) | {nm + "_nan" for nm in names}


@pytest.mark.parametrize("merged", [False, True], ids=["own_clusters", "cluster_keys"])
def test_keyed_evaluation_and_human_ceiling(merged):
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    M = S()
    gt, pr, gt_keys, pr_keys = _keyed_case()
    keys = ["d", "c", "f", "b", "e", "a"]                              # first-appearance order of gt_keys
    assert [gt_keys.count(k) for k in keys] == [4, 3, 3, 2, 2, 1] and [pr_keys.count(k) for k in keys] == [1, 3, 1, 0, 2, 2]
    h, gap = 20.0, -0.25
    image = {k: ("ef" if merged and k in "ef" else k) for k in keys}
    cluster_keys = [image[k] for k in gt_keys] if merged else None
    pooled = {im: np.concatenate([gt[i][:, :2] for i in range(len(gt)) if image[gt_keys[i]] == im], 0) for im in set(image.values())}
    ims = sorted(pooled)
    centres_of_image = dict(zip(ims, [c for c, _, _ in M.meanshift_clusters([pooled[im] for im in ims], bandwidth=h)]))
    centres_of = {k: centres_of_image[image[k]] for k in keys}
    assert all(len(c) >= 1 for c in centres_of.values()) and max(len(c) for c in centres_of.values()) >= 3
    groups = {k: [(j, gt[i], pr[j]) for j in range(len(pr)) if pr_keys[j] == k for i in range(len(gt)) if gt_keys[i] == k] for k in keys}
    names, want = _by_definition(M, groups, centres_of, gap)
    L = hip.lib()
    calls = {}
    originals = {n: getattr(L, n) for n in ("sp_meanshift", "sp_scan_cluster_strings", "sp_scan_sequence")}
    for n, fn in originals.items():
        def counted(*args, _n=n, _fn=fn):
            calls[_n] = calls.get(_n, 0) + 1
            return _fn(*args)
        setattr(L, n, counted)
    try:
        means, per_key = E.sequence_score_evaluation(gt, pr, gt_keys, pr_keys, bandwidth=h, gap=gap, cluster_keys=cluster_keys)
    finally:
        for n, fn in originals.items():
            setattr(L, n, fn)
    assert calls == {"sp_meanshift": 1, "sp_scan_cluster_strings": 1, "sp_scan_sequence": 1}      # the whole call is one batch
    _check_tables(means, per_key, names, want, keys)
    b = keys.index("b")
    assert all(np.isnan(per_key[nm][b]) for nm in names) and means["SS_nan"] == 1                 # the key without predictions
    rest = [k for k in range(len(keys)) if k != b]
    assert not np.isnan(per_key["SS"][rest]).any()
    assert (per_key["SS_best"][rest] >= per_key["SS"][rest]).all() and (per_key["FED_best"][rest] <= per_key["FED"][rest]).all()
    # the human ceiling: every ordered pair of distinct human scanpaths of a key, the second as the "prediction"
    groups = {k: [(j, gt[i], gt[j]) for j in range(len(gt)) if gt_keys[j] == k for i in range(len(gt)) if gt_keys[i] == k and i != j]
              for k in keys}
    names, want = _by_definition(M, groups, centres_of, gap)
    means, per_key = E.sequence_score_human_evaluation(gt, gt_keys, bandwidth=h, gap=gap, cluster_keys=cluster_keys)
    _check_tables(means, per_key, names, want, keys)
    a = keys.index("a")
    assert all(np.isnan(per_key[nm][a]) for nm in names) and means["FED_nan"] == 1                # the key with one human scanpath
    # one measure alone, default gap: against the checker end to end
    means, per_key = E.sequence_score_evaluation(gt, pr, gt_keys, pr_keys, bandwidth=h, metrics=("FED",), cluster_keys=cluster_keys)
    assert set(per_key) == {"keys", "FED", "FED_best"}
    want = []
    for k in keys:
        cen = R.meanshift(pooled[image[k]], h)[0]
        v = [R.fixation_edit_distance(R.labels_of(gt[i], cen), R.labels_of(pr[j], cen)) for j in range(len(pr)) if pr_keys[j] == k
             for i in range(len(gt)) if gt_keys[i] == k]
        want.append(np.mean(v) if v else np.nan)
    assert np.array_equal(per_key["FED"], np.array(want), equal_nan=True)
