"""csrc/scandist.hip through scanpath_distances_pairs, the per-pair wrappers, the C entry points and the keyed evaluations, against the
Python checker tests/scanpath_dist_ref.py -- float64, BIT FOR BIT (np.array_equal with equal_nan): the arithmetic is IEEE add, multiply,
square root, divide, compare and integer counting, so a differing bit is a contraction or a wrong summation order, not a margin."""
import os

import numpy as np
import pytest
import torch

import scanpath_dist_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ALL = R.DISTANCES + R.RECURRENCE
LENGTHS = (0, 1, 2, 3, 5, 31, 32, 33, 63, 64)
SQUARE = np.array([[100.0, 100.0], [200.0, 100.0], [200.0, 200.0], [100.0, 200.0]])
_REF = {}


def M():
    from scanpaths_amd.utils.evaltools import visual_attention_metrics
    return visual_attention_metrics


def ref(tag, paths, pairs, max_dim=1.0, radius=None, min_line=2, metrics=ALL):
    """the checker's scores, computed once per distinct call and shared (read-only) among the tests"""
    key = (tag, float(max_dim), radius, min_line, tuple(metrics))
    if key not in _REF:
        _REF[key] = R.score_pairs(paths, pairs, metrics, max_dim, radius, min_line)
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


def same(got, want, what=""):
    assert list(got) == list(want), (what, list(got), list(want))
    for m in want:
        a, b = np.asarray(got[m]), np.asarray(want[m])
        assert a.dtype == np.float64 and a.shape == b.shape, (what, m, a.dtype, a.shape, b.shape)
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        print(f"{what} {m}: {int(bad.sum())} of {a.size} differ")
        assert np.array_equal(a, b, equal_nan=True), (what, m, np.flatnonzero(bad)[:8], a[bad][:8], b[bad][:8])


def grid_paths(lengths, seed, ncol=2, cells=12):
    """coordinates on an 8-pixel grid (minima tie, distances repeat); columns beyond x, y hold values that must not be read"""
    g = np.random.Generator(np.random.PCG64(seed))
    xy = [g.integers(0, cells, (n, 2)) * 8.0 for n in lengths]
    return [np.concatenate([a, g.uniform(-1e3, 1e3, (len(a), ncol - 2))], 1) for a in xy]


@pytest.mark.parametrize("ncol", [2, 3, 5])
def test_lengths_where_indexing_breaks(ncol):
    """all ordered pairs among lengths 0 .. 64, self-pairs (the same index on both sides) included"""
    paths = grid_paths(LENGTHS, 1, ncol)
    pairs = [(a, b) for a in range(len(LENGTHS)) for b in range(len(LENGTHS))]
    got = M().scanpath_distances_pairs(paths, pairs, metrics=ALL, radius=16.0)
    want = ref("lengths", grid_paths(LENGTHS, 1), pairs, radius=16.0)
    same(got, want, f"lengths ncol={ncol}")
    k = pairs.index((9, 9))                                        # 64 x 64 against itself
    assert got["DTW"][k] == 0.0 and got["DET"][k] > 0.0 and got["CORM"][k] == 0.0
    empty = [k for k, (a, b) in enumerate(pairs) if LENGTHS[a] == 0 or LENGTHS[b] == 0]
    assert all(np.isnan(got[m][empty]).all() for m in ALL) and not np.isnan(np.delete(got["DTW"], empty)).any()


@pytest.mark.parametrize("npairs", [1, 63, 64, 65, 130])
def test_pair_counts(npairs):
    """one launch each; the pairs repeat and come out of order (four pairs share a block: 1, 63 and 65 leave waves without a pair)"""
    paths = grid_paths((0, 1, 2, 4, 7, 9, 12, 17), 2, ncol=3)
    g = np.random.Generator(np.random.PCG64(100 + npairs))
    pairs = g.integers(0, len(paths), (npairs, 2))
    pairs[npairs // 2:] = pairs[:npairs - npairs // 2][::-1]        # repeats, reversed
    got = M().scanpath_distances_pairs(paths, pairs, metrics=ALL, radius=12.0, min_line=3)
    same(got, R.score_pairs(paths, pairs, ALL, 1.0, 12.0, 3), f"npairs={npairs}")


def test_each_output_alone_and_all_together_and_repeat_runs():
    paths = grid_paths((0, 1, 3, 6, 11, 20, 33, 64), 3)
    pairs = [(a, b) for a in range(8) for b in range(8)]
    V = M()
    both = V.scanpath_distances_pairs(paths, pairs, metrics=ALL, radius=16.0)
    same(both, ref("alone", paths, pairs, radius=16.0), "all together")
    for m in ALL:
        one = V.scanpath_distances_pairs(paths, pairs, metrics=(m,), radius=16.0 if m in R.RECURRENCE else None)
        same(one, {m: both[m]}, f"{m} alone")
    rev = V.scanpath_distances_pairs(paths, pairs, metrics=ALL[::-1], radius=16.0)             # the caller's order of metrics
    assert list(rev) == list(ALL[::-1])
    for _ in range(3):
        same(V.scanpath_distances_pairs(paths, pairs, metrics=ALL, radius=16.0), both, "repeat run")
    same({m: rev[m] for m in ALL}, both, "reversed metrics")


@pytest.mark.parametrize("max_dim", [1.0, 320.0])
def test_max_dim(max_dim):
    g = np.random.Generator(np.random.PCG64(4))
    paths = [np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.1, 0.5, n)], 1) for n in (1, 2, 5, 9, 14, 16, 23)]
    paths += grid_paths((3, 8, 15), 5, ncol=3, cells=30)
    pairs = [(a, b) for a in range(len(paths)) for b in range(len(paths))]
    radius = 32.0 / max_dim                                         # on the grid paths d = 32 px happens: the <= edge after scaling
    got = M().scanpath_distances_pairs(paths, pairs, metrics=ALL, max_dim=max_dim, radius=radius)
    same(got, ref("max_dim", paths, pairs, max_dim, radius), f"max_dim={max_dim}")


@pytest.mark.parametrize("min_line", [2, 3])
@pytest.mark.parametrize("radius", [8.0, 12.0, 40.0])              # 8 = one cell, 40 = the 24-32-40 triangle: d == radius exactly
def test_recurrence_parameters(radius, min_line):
    paths = grid_paths((1, 2, 3, 4, 7, 12, 19, 32, 33), 6, cells=8)
    paths += [SQUARE, SQUARE[::-1].copy(), np.repeat(SQUARE[:1], 4, 0), SQUARE + 500.0]
    n = len(paths)
    pairs = [(a, b) for a in range(n) for b in range(n)]
    got = M().scanpath_distances_pairs(paths, pairs, metrics=R.RECURRENCE, radius=radius, min_line=min_line)
    want = ref("recurrence", paths, pairs, 1.0, radius, min_line, R.RECURRENCE)
    same(got, want, f"radius={radius} min_line={min_line}")
    at = lambda a, b: tuple(got[m][pairs.index((a, b))] for m in R.RECURRENCE)
    sq = n - 4
    if min_line == 2:
        assert at(sq, sq) == (25.0, 100.0, 0.0, 0.0)                                  # P = Q
        assert at(sq, sq + 1)[:2] == (25.0, 0.0)                                      # Q = P reversed
        assert at(sq, sq + 2) == (25.0, 0.0, 50.0, 50.0)                              # Q = four copies of P[0]
    r0 = at(sq, sq + 3)                                                               # no recurrent point: R = 0
    assert r0[0] == 0.0 and all(np.isnan(v) for v in r0[1:])
    n1 = at(0, sq)                                                                    # N = 1
    assert n1[0] in (0.0, 100.0) and np.isnan(n1[3]) and (n1[0] == 0.0) == np.isnan(n1[1])
    edge = [k for k, (a, b) in enumerate(pairs) if any(v == radius for row in R.dist_matrix(paths[a], paths[b])[0] for v in row)]
    assert radius == 12.0 or len(edge) > 10, "d == radius must occur for the <= edge to be exercised"


def test_distances_sanity_values_and_wrappers():
    V = M()
    assert (V.DTW(SQUARE, SQUARE), V.frechet_distance(SQUARE, SQUARE), V.hausdorff_distance(SQUARE, SQUARE),
            V.eyenalysis_distance(SQUARE, SQUARE)) == (0.0, 0.0, 0.0, 0.0)
    assert V.cross_recurrence(SQUARE, SQUARE, radius=10) == {"REC": 25.0, "DET": 100.0, "LAM": 0.0, "CORM": 0.0}
    P = np.array([[0.0, 0.0, 0.2], [4.0, 0.0, 0.3], [8.0, 0.0, 0.1]])
    Q = np.array([[0.0, 3.0, 0.2], [4.0, 3.0, 0.2], [8.0, 3.0, 0.2], [12.0, 3.0, 0.2]])
    assert (V.DTW(P, Q), V.frechet_distance(P, Q), V.hausdorff_distance(P, Q), V.eyenalysis_distance(P, Q)) == (14.0, 5.0, 5.0, 5.75)
    assert V.cross_recurrence(P, Q, radius=5.0, min_line=3) == dict(zip(R.RECURRENCE, R.cross_recurrence(P, Q, 5.0, 3)))
    assert np.isnan(V.DTW([], Q)) and np.isnan(V.eyenalysis_distance(P, np.zeros((0, 3))))
    assert all(np.isnan(v) for v in V.cross_recurrence(P, [], radius=5.0).values())


def _unrag(npz, name):
    cat, off = npz[name].reshape(-1, 3), npz[name + "_off"]       # offsets count fixations
    return [cat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_real_scanpaths():
    V = M()
    ex = _unrag(np.load(os.path.join(GOLD, "scanmatch.npz")), "ex_fix")          # the reference's three example scanpaths
    assert [len(e) for e in ex] == [19, 16, 20]
    pairs = [(a, b) for a in range(3) for b in range(3)]
    got = V.scanpath_distances_pairs(ex, pairs, metrics=ALL, radius=64.0)
    same(got, ref("ex", ex, pairs, radius=64.0), "example scanpaths")
    got = V.scanpath_distances_pairs(ex, pairs, metrics=ALL, max_dim=1024.0, radius=0.0625)
    same(got, ref("ex", ex, pairs, 1024.0, 0.0625), "example scanpaths / 1024")
    rnd = _unrag(np.load(os.path.join(GOLD, "sed_stde.npz")), "rnd_fix")
    assert len(rnd) == 40
    pairs = [(a, b) for a in range(40) for b in range(40)]
    got = V.scanpath_distances_pairs(rnd, pairs, metrics=ALL, radius=30.0)
    same(got, ref("rnd", rnd, pairs, radius=30.0), "40 random scanpaths")
    d = got["DTW"].reshape(40, 40)
    assert np.array_equal(d, d.T) and np.array_equal(got["CORM"].reshape(40, 40), -got["CORM"].reshape(40, 40).T, equal_nan=True)
    assert (got["Hausdorff"] <= got["Frechet"]).all() and (got["Frechet"] <= got["DTW"]).all()


def test_kernel_guards_itself_against_a_scanpath_beyond_the_limit():
    """the C entry points directly: a count of 65 gives NaN in every output of its pairs; the other pairs of the launch are unaffected"""
    from scanpaths_amd import hip
    L = hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    assert L.sp_scan_max_fixations() == 64
    paths = grid_paths((5, 65, 7, 64), 7, ncol=3)
    counts = [len(a) for a in paths]
    fix = torch.from_numpy(np.concatenate(paths, 0)).to(dev)
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    start = torch.tensor(np.cumsum([0] + counts[:-1]), dtype=torch.int64, device=dev)
    pairs = [(0, 2), (0, 1), (1, 2), (3, 3), (1, 1), (2, 0), (3, 1), (2, 3), (0, 0)]
    pr = torch.tensor(pairs, dtype=torch.int32, device=dev)
    n = len(pairs)
    out_d = torch.full((4, n), 7.0, dtype=torch.float64, device=dev)
    rec_d = torch.full((n, 4), 7.0, dtype=torch.float64, device=dev)
    hip.check(L.sp_scan_distances(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, 1.0, out_d[0].data_ptr(),
                                  out_d[1].data_ptr(), out_d[2].data_ptr(), out_d[3].data_ptr(), hip.stream()), "sp_scan_distances")
    hip.check(L.sp_scan_recurrence(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, 1.0, 16.0, 2, hip.ptr(rec_d),
                                   hip.stream()), "sp_scan_recurrence")
    torch.cuda.synchronize()
    out, rec = out_d.cpu().numpy(), rec_d.cpu().numpy()
    bad = np.array([1 in p for p in pairs])
    assert np.isnan(out[:, bad]).all() and np.isnan(rec[bad]).all()
    ok = [p for p in pairs if 1 not in p]
    safe = [paths[0], np.zeros((0, 3)), paths[2], paths[3]]
    want = R.score_pairs(safe, ok, ALL, 1.0, 16.0, 2)
    same({m: out[k, ~bad] for k, m in enumerate(R.DISTANCES)}, {m: want[m] for m in R.DISTANCES}, "neighbours of the guarded pairs")
    same({m: rec[~bad, k] for k, m in enumerate(R.RECURRENCE)}, {m: want[m] for m in R.RECURRENCE}, "neighbours of the guarded pairs")
    # the launchers' argument checks on a live device
    assert L.sp_scan_distances(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, 1.0, None, None, None, None, hip.stream()) == -2
    assert L.sp_scan_recurrence(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(pr), n, 1.0, 16.0, 1, hip.ptr(rec_d), hip.stream()) == -1


def _keyed_case():
    """4 keys, 1 .. 4 human scanpaths and 0 .. 3 predictions each, interleaved: "b" has no prediction, "a" one human scanpath"""
    g = np.random.Generator(np.random.PCG64(8))

    def path():
        n = int(g.integers(2, 9))
        return np.stack([g.integers(0, 5, n) * 16.0, g.integers(0, 4, n) * 16.0, g.uniform(0.1, 0.5, n)], 1)

    humans = {"a": 1, "b": 2, "c": 3, "d": 4}
    preds = {"a": 2, "b": 0, "c": 3, "d": 1}
    gt_keys = [k for r in range(4) for k in "dcba" if r < humans[k]]
    pr_keys = [k for r in range(3) for k in "acd" if r < preds[k]]
    return [path() for _ in gt_keys], [path() for _ in pr_keys], gt_keys, pr_keys


def _nanmean(v):
    """the mean of the values that are not NaN, NaN if there is none"""
    v = np.array([x for x in v if not np.isnan(x)], dtype=np.float64)
    return v.mean() if v.size else np.nan


def _by_definition(V, groups, radius):
    """groups: key -> list of (prediction id, human scanpath, predicted scanpath); the per-pair wrappers, one pair at a time"""
    names = list(ALL) + [m + "_best" for m in ALL if m != "CORM"]
    per_key = {nm: [] for nm in names}
    for key, trip in groups.items():
        rows = {}
        for j, h, p in trip:
            r = {"DTW": V.DTW(h, p), "Frechet": V.frechet_distance(h, p), "Hausdorff": V.hausdorff_distance(h, p),
                 "Eyenalysis": V.eyenalysis_distance(h, p)}
            r.update(V.cross_recurrence(h, p, radius=radius))
            rows.setdefault(j, []).append(r)
        for m in ALL:
            flat = [r[m] for rs in rows.values() for r in rs]
            per_key[m].append(_nanmean(flat))
            if m != "CORM":
                pick = min if m in R.DISTANCES else max
                best = [pick([r[m] for r in rs if not np.isnan(r[m])], default=np.nan) for rs in rows.values()]
                per_key[m + "_best"].append(_nanmean(best))
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


def test_keyed_evaluation_and_human_ceiling():
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    V = M()
    gt, pr, gt_keys, pr_keys = _keyed_case()
    keys = ["d", "c", "b", "a"]                                     # first-appearance order of gt_keys
    assert [gt_keys.count(k) for k in keys] == [4, 3, 2, 1] and [pr_keys.count(k) for k in keys] == [1, 3, 0, 2]
    radius = 24.0
    groups = {k: [(j, gt[i][:, :2], pr[j][:, :2]) for j in range(len(pr)) if pr_keys[j] == k for i in range(len(gt)) if gt_keys[i] == k]
              for k in keys}
    names, want = _by_definition(V, groups, radius)
    L = hip.lib()
    calls = {}
    originals = {n: getattr(L, n) for n in ("sp_scan_distances", "sp_scan_recurrence")}
    for n, fn in originals.items():
        def counted(*args, _n=n, _fn=fn):
            calls[_n] = calls.get(_n, 0) + 1
            return _fn(*args)
        setattr(L, n, counted)
    try:
        means, per_key = E.scanpath_distance_evaluation(gt, pr, gt_keys, pr_keys, metrics=ALL, radius=radius)
    finally:
        for n, fn in originals.items():
            setattr(L, n, fn)
    assert calls == {"sp_scan_distances": 1, "sp_scan_recurrence": 1}                 # the whole call is one batch
    _check_tables(means, per_key, names, want, keys)
    b = keys.index("b")
    assert all(np.isnan(per_key[nm][b]) for nm in names) and means["DTW_nan"] == 1    # the key without predictions
    assert not np.isnan(per_key["DTW"][[0, 1, 3]]).any()
    assert (per_key["DTW_best"][[0, 1, 3]] <= per_key["DTW"][[0, 1, 3]]).all() and (per_key["REC_best"][[0, 1, 3]] >= per_key["REC"][[0, 1, 3]]).all()
    # the human ceiling: every ordered pair of distinct human scanpaths of a key, the second as the "prediction"
    groups = {k: [(j, gt[i][:, :2], gt[j][:, :2]) for j in range(len(gt)) if gt_keys[j] == k for i in range(len(gt))
                  if gt_keys[i] == k and i != j] for k in keys}
    names, want = _by_definition(V, groups, radius)
    means, per_key = E.scanpath_distance_human_evaluation(gt, gt_keys, metrics=ALL, radius=radius)
    _check_tables(means, per_key, names, want, keys)
    a = keys.index("a")
    assert all(np.isnan(per_key[nm][a]) for nm in names) and means["Frechet_nan"] == 1   # the key with one human scanpath
    # a subset of the measures, without a radius
    means, per_key = E.scanpath_distance_evaluation(gt, pr, gt_keys, pr_keys, metrics=("Hausdorff", "DTW"))
    assert set(per_key) == {"keys", "Hausdorff", "Hausdorff_best", "DTW", "DTW_best"}
    want = []
    for k in keys:
        v = [R.dtw(gt[i], pr[j]) for j in range(len(pr)) if pr_keys[j] == k for i in range(len(gt)) if gt_keys[i] == k]
        want.append(np.mean(v) if v else np.nan)
    assert np.array_equal(per_key["DTW"], np.array(want), equal_nan=True)
