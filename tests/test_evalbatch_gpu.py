"""One edge batch through every evaluation scorer that packs its scanpaths with evaltools/_batch.py: 5 scanpaths (an odd
number: the int32 counts end off an 8-byte boundary) of 3, 1, 64, 2 and 5 fixations with 3 columns, and 3 pairs (odd again) -- one with
the 64-fixation scanpath (the lane limit), one of a scanpath with itself, one with a scanpath of fewer than 3 fixations (the MultiMatch
gate, the k loops).  A second form has an empty scanpath in front, for the scorers that take one.  Every scorer is compared with the
host checker and at the bar of its own test file: no bar is new here.

  sed_stde_pairs            oracle/metrics_oracle.py: SED equal, STDE within 4 ulp      (test_scanmatch_gpu)
  tde_pairs                 the reference's loops restated below, 1e-12                  (test_salmaps_gpu, there against the golden file)
  scanpath_distances_pairs  tests/scanpath_dist_ref.py, bit for bit                      (test_scanpath_distances_gpu)
  multimatch_pairs          docomparison: 1e-13, direction 1e-12, the same NaNs          (test_dataset_eval_gpu, test_multimatch_simplify_gpu)
  simplify_scanpaths        simplify_scanpath, bit for bit                               (test_multimatch_simplify_gpu)
  sequence_score            tests/seqscore_ref.py, bit for bit                           (test_sequence_score_gpu)
  ScanMatch.sequences       oracle/scanmatch_oracle.py, bit for bit                      (test_scanmatch_gpu)
  fixation_maps             np.add.at with the pixel rule, bit for bit                   (test_fixmaps_gpu, there against the golden file)

A second, off-grid batch (22 scanpaths of 1 .. 64 fixations, ~300 pairs) holds what csrc/scan_common.h states for the kernels of
scanmetrics.hip: tde_pairs and euclidean_distance equal numpy's plain loops BIT FOR BIT (a product fused into the sum shows only off
the pixel grid: with the fused product 6 .. 28 of the 294 pairs differed per call), STDE and MultiMatch keep their bars there, and
the three kernels answer a count outside [0, 64] with NaN / -1 instead of indexing their per-thread arrays with it."""
import numpy as np
import pytest
import torch

import scanpath_dist_ref as DR
import seqscore_ref as SR
from oracle import metrics_oracle as MO
from oracle import scanmatch_oracle as SO

pytestmark = pytest.mark.gpu
LENGTHS = (3, 1, 64, 2, 5)
PAIRS = [(2, 4), (0, 0), (1, 4)]
SHAPE = (240, 320, 3)
TRIPLE = dict(TDir=45.0, TDur=0.3, TAmp=40.0)


def _batch():
    g = np.random.default_rng(2026)
    return [np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.05, 0.4, n)], 1) for n in LENGTHS]


FORMS = {"plain": (_batch(), PAIRS),
         "empty first": ([np.zeros((0, 3))] + _batch(), [(a + 1, b + 1) for a, b in PAIRS[:2]] + [(0, 5)])}
FORM = pytest.mark.parametrize("form", list(FORMS))


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (what, got, want)


def _tde_k(H, S, k, mode="Mean"):
    """time_delay_embedding_distance of the reference at one k in plain loops (H, S already divided by max_dim); NaN where it
    returns False"""
    if len(H) < k or len(S) < k:
        return float("nan")
    dists = []
    for s0 in range(len(S) - k + 1):
        d = [np.sqrt((S[s0:s0 + k, 0] - H[h0:h0 + k, 0]) ** 2 + (S[s0:s0 + k, 1] - H[h0:h0 + k, 1]) ** 2).sum()
             for h0 in range(len(H) - k + 1)]
        dists.append(min(d) / k)
    return float(sum(dists) / len(dists) if mode == "Mean" else max(dists))


def _tde(human, simulated, max_dim):
    """scaled_time_delay_embedding_distance of the reference in plain loops: the mean over k = 1 .. min(n, m) of the 'Mean' mode
    time_delay_embedding_distance (oracle/metrics_oracle.stde without its exp); NaN where the reference returns None"""
    H, S = human[:, :2] / max_dim, simulated[:, :2] / max_dim
    kmax = min(len(H), len(S))
    if kmax == 0:
        return float("nan")
    per_k = [_tde_k(H, S, k) for k in range(1, kmax + 1)]
    return float(sum(per_k) / len(per_k))


def _euclidean(human, simulated):
    """euclidean_distance of the reference; NaN where it returns False"""
    if len(human) != len(simulated):
        return float("nan")
    return float(np.sqrt((human[:, 0] - simulated[:, 0]) ** 2 + (human[:, 1] - simulated[:, 1]) ** 2).sum())


@FORM
def test_sed_stde_and_tde(form):
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    paths, pairs = FORMS[form]
    sed, stde = M.sed_stde_pairs(paths, pairs, SHAPE)
    assert sed.is_cuda and sed.dtype == torch.int32 and stde.is_cuda and stde.dtype == torch.float64
    sed, stde = sed.cpu().numpy(), stde.cpu().numpy()
    want_sed = np.array([MO.sed(SHAPE, paths[a], paths[b]) for a, b in pairs], dtype=np.int32)
    want = np.array([MO.stde(paths[a], paths[b], SHAPE) for a, b in pairs])
    print(form, "SED", sed, want_sed, "STDE", stde, want)
    _same(sed, want_sed, "SED")
    assert np.array_equal(np.isnan(stde), np.isnan(want)) and np.all(np.abs(stde - want)[~np.isnan(want)] <= 4 * np.spacing(want[~np.isnan(want)]))
    tde, eucl = M.tde_pairs(paths, pairs, k=0, max_dim=320.0, want_euclidean=True)
    tde, eucl = tde.cpu().numpy(), eucl.cpu().numpy()
    for p, (a, b) in enumerate(pairs):
        r = _tde(paths[a], paths[b], 320.0)
        assert (np.isnan(tde[p]) and np.isnan(r)) or abs(tde[p] - r) <= 1e-12, (form, a, b, tde[p], r)
        assert np.isnan(eucl[p]) == (len(paths[a]) != len(paths[b])), (form, a, b, eucl[p])
    assert eucl[1] == 0.0                                              # the self-pair


# ---- off the pixel grid: dx*dx is inexact, so a product fused into the sum shows in the last bit (csrc/scan_common.h) ----
OFF_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64)     # both branches of numpy's summation scheme, its remainder loop, the limit


def _offgrid():
    """two seeded scanpaths of every length (index 2 i and 2 i + 1 have OFF_LENGTHS[i] fixations) and two pair lists.  all: the 44
    equal-length pairs (where euclidean_distance is defined), 240 drawn among the scanpaths of <= 17 fixations, 10 that mix a long one
    with a short one -- 294.  k0, for the O(n^4) sum over every k: the same without the long equal-length pairs but (64, 64) once;
    four of its pairs involve a 64-fixation scanpath."""
    g = np.random.default_rng(950)
    paths = [np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.05, 0.4, n)], 1) for n in OFF_LENGTHS for _ in range(2)]
    K, short = len(paths), 18
    equal = [(a, b) for a in range(K) for b in range(K) if len(paths[a]) == len(paths[b])]
    drawn = [(int(a), int(b)) for a, b in g.integers(0, short, (240, 2))]
    mixed = [(18, 3), (5, 19), (19, 12), (16, 18), (18, 9), (10, 19), (20, 4), (9, 21), (21, 17), (0, 20)]
    k0 = [p for p in equal if max(p) < short] + drawn + mixed[:-1] + [(20, 21)]
    assert sum(1 for p in k0 if max(p) >= 20) == 4
    return paths, equal + drawn + mixed, k0


OFF_PATHS, OFF_PAIRS, OFF_PAIRS_K0 = _offgrid()


@pytest.mark.parametrize("k,mode", [(k, m) for k in (1, 2, 3, 8) for m in ("Mean", "Hausdorff")] + [(0, "Mean")])
def test_tde_and_euclidean_are_numpys_bit_for_bit_off_the_grid(k, mode):
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    pairs, max_dim = (OFF_PAIRS_K0, 320.0) if k == 0 else (OFF_PAIRS, 1.0)
    tde, eucl = M.tde_pairs(OFF_PATHS, pairs, k=k, distance_mode=mode, max_dim=max_dim, want_euclidean=True)
    tde, eucl = tde.cpu().numpy(), eucl.cpu().numpy()
    if k == 0:
        want = np.array([_tde(OFF_PATHS[a], OFF_PATHS[b], max_dim) for a, b in pairs])
    else:
        want = np.array([_tde_k(OFF_PATHS[a][:, :2] / max_dim, OFF_PATHS[b][:, :2] / max_dim, k, mode) for a, b in pairs])
    want_eucl = np.array([_euclidean(OFF_PATHS[a], OFF_PATHS[b]) for a, b in pairs])
    differ = lambda x, y: int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum())
    print(f"k={k} {mode}: TDE {differ(tde, want)} of {len(pairs)} pairs differ, Euclidean {differ(eucl, want_eucl)}")
    assert (~np.isnan(want)).sum() >= 50 and (~np.isnan(want_eucl)).sum() >= 36
    _same(eucl, want_eucl, ("Euclidean", k, mode))
    _same(tde, want, ("TDE", k, mode))


def test_stde_off_the_grid():
    """the exponent is held bit for bit by the test above; exp()'s last bit is the device library's, so STDE keeps the 4-ulp bar"""
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    _, stde = M.sed_stde_pairs(OFF_PATHS, OFF_PAIRS_K0, SHAPE, want_sed=False)
    stde = stde.cpu().numpy()
    want = np.array([MO.stde(OFF_PATHS[a], OFF_PATHS[b], SHAPE) for a, b in OFF_PAIRS_K0])
    assert not np.isnan(want).any() and not np.isnan(stde).any()
    ulps = np.abs(stde - want) / np.spacing(want)
    print(f"STDE: largest distance to the oracle {ulps.max()} ulp, {int((ulps > 0).sum())} of {len(want)} pairs differ")
    assert ulps.max() <= 4


def test_multimatch_off_the_grid():
    from scanpaths_amd.utils.evaltools.multimatch import docomparison, multimatch_pairs
    dev = multimatch_pairs(OFF_PATHS, OFF_PAIRS, [320, 240])
    with np.errstate(all="ignore"):
        ref = np.array([docomparison(OFF_PATHS[a], OFF_PATHS[b], screensize=[320, 240]) for a, b in OFF_PAIRS], dtype=np.float64)
    assert dev.shape == ref.shape == (len(OFF_PAIRS), 5) and np.array_equal(np.isnan(ref), np.isnan(dev))
    nan = np.isnan(ref).any(1)
    assert nan.tolist() == [min(len(OFF_PATHS[a]), len(OFF_PATHS[b])) < 3 for a, b in OFF_PAIRS] and (~nan).sum() > 100
    worst = np.abs(ref[~nan] - dev[~nan]).max(0)
    print("MultiMatch: largest difference to docomparison per column", worst)
    assert (worst[[0, 2, 3, 4]] <= 1e-13).all() and worst[1] <= 1e-12, worst


def test_the_pair_kernels_of_scanmetrics_guard_themselves():
    """the C entry points directly, with counts that lie: 65 and -1 give NaN (sed: -1) in every output of their pairs and none of
    their rows is read; the other pairs of the launch equal the scorers' results without those scanpaths"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    from scanpaths_amd.utils.evaltools.multimatch import multimatch_pairs
    L = hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = np.random.default_rng(65)
    counts = [5, 65, 7, -1, 64]
    paths = [np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.05, 0.4, n)], 1) for n in (5, 65, 7, 0, 64)]
    fix = torch.from_numpy(np.concatenate(paths, 0)).to(dev)
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    gate = torch.full((5,), 10, dtype=torch.int32, device=dev)
    start = torch.tensor(np.cumsum([0] + [len(a) for a in paths[:-1]]), dtype=torch.int64, device=dev)
    pairs = [(0, 2), (0, 1), (1, 2), (4, 4), (1, 1), (2, 0), (4, 1), (2, 4), (0, 0), (3, 0), (2, 3), (3, 3), (3, 1)]
    pr = torch.tensor(pairs, dtype=torch.int32, device=dev)
    n = len(pairs)
    sed = torch.full((n,), 7, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)
    stde, tde0, tde3, eucl, mm, mmg = f64(n), f64(n), f64(n), f64(n), f64(n, 5), f64(n, 5)
    args = (hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count))
    hip.check(L.sp_scan_sed_stde(*args, hip.ptr(pr), n, 240, 320, 5, 320.0, hip.ptr(sed), hip.ptr(stde), hip.stream()), "sp_scan_sed_stde")
    hip.check(L.sp_scan_tde(*args, hip.ptr(pr), n, 0, 0, 320.0, hip.ptr(tde0), hip.ptr(eucl), hip.stream()), "sp_scan_tde")
    hip.check(L.sp_scan_tde(*args, hip.ptr(pr), n, 3, 1, 1.0, hip.ptr(tde3), None, hip.stream()), "sp_scan_tde")
    hip.check(L.sp_scan_multimatch(*args, hip.ptr(pr), n, 320.0, 240.0, hip.ptr(mm), hip.stream()), "sp_scan_multimatch")
    hip.check(L.sp_scan_multimatch_gated(*args, hip.ptr(gate), hip.ptr(pr), n, 320.0, 240.0, hip.ptr(mmg), hip.stream()),
              "sp_scan_multimatch_gated")
    torch.cuda.synchronize()
    bad = np.array([1 in p or 3 in p for p in pairs])
    assert bad.sum() == 8 and (sed.cpu().numpy()[bad] == -1).all()
    for out in (stde, tde0, tde3, eucl, mm, mmg):
        assert np.isnan(out.cpu().numpy()[bad]).all()
    ok = [p for p in pairs if 1 not in p and 3 not in p]
    safe = [paths[0], np.zeros((0, 3)), paths[2], np.zeros((0, 3)), paths[4]]
    want_sed, want_stde = M.sed_stde_pairs(safe, ok, SHAPE)
    want0, want_eucl = M.tde_pairs(safe, ok, k=0, max_dim=320.0, want_euclidean=True)
    want3, _ = M.tde_pairs(safe, ok, k=3, distance_mode="Hausdorff")
    want_mm = multimatch_pairs(safe, ok, [320, 240])
    for got, want, what in ((sed, want_sed, "SED"), (stde, want_stde, "STDE"), (tde0, want0, "TDE k=0"), (eucl, want_eucl, "Euclidean"),
                            (tde3, want3, "TDE k=3"), (mm, want_mm, "MultiMatch"), (mmg, want_mm, "MultiMatch, gated")):
        _same(got.cpu().numpy()[~bad], want.cpu().numpy() if torch.is_tensor(want) else want, what)
    assert not np.isnan(want_mm).any() and not np.isnan(want0.cpu().numpy()).any()


def test_an_empty_scanpath_scores_the_other_ones_length_and_nan():
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    paths = FORMS["empty first"][0]
    sed, stde = M.sed_stde_pairs(paths, [(0, 3), (3, 0), (0, 0)], SHAPE)
    assert sed.cpu().tolist() == [64, 64, 0] and torch.isnan(stde).all()
    assert M.string_edit_distance(np.zeros(SHAPE), [], paths[5]) == 5 == M.string_edit_distance(np.zeros(SHAPE), paths[5], [])
    assert M.scaled_time_delay_embedding_similarity([], paths[5], np.zeros(SHAPE)) is None
    assert [t.shape[0] for t in M.sed_stde_pairs([], [], SHAPE)] == [0, 0]


@FORM
def test_scanpath_distances(form):
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    paths, pairs = FORMS[form]
    metrics = DR.DISTANCES + DR.RECURRENCE
    got = M.scanpath_distances_pairs(paths, pairs, metrics=metrics, radius=16.0)
    want = DR.score_pairs(paths, pairs, metrics, 1.0, 16.0, 2)
    assert list(got) == list(want)
    for m in want:
        _same(got[m], want[m], (form, m))
    one = M.scanpath_distances_pairs(paths, pairs, metrics=("Hausdorff",))          # a single odd-length result section
    _same(one["Hausdorff"], want["Hausdorff"], (form, "alone"))


@FORM
def test_multimatch_and_simplification(form):
    from scanpaths_amd.utils.evaltools.multimatch import docomparison, multimatch_pairs, simplify_scanpath, simplify_scanpaths
    paths, pairs = FORMS[form]
    got = simplify_scanpaths(paths, **TRIPLE)
    assert len(got) == len(paths)
    for k, p in enumerate(paths):
        _same(got[k], simplify_scanpath(p, *TRIPLE.values()), (form, "simplify", k))
    assert len(got[-3]) < 64                                           # the long scanpath did get shorter
    for kw in ({}, dict(grouping=True, **TRIPLE)):
        dev = multimatch_pairs(paths, pairs, [320, 240], **kw)
        with np.errstate(all="ignore"):
            ref = np.array([docomparison(paths[a], paths[b], screensize=[320, 240], **kw) for a, b in pairs], dtype=np.float64)
        print(form, kw, dev, ref)
        assert dev.shape == ref.shape == (3, 5) and np.array_equal(np.isnan(ref), np.isnan(dev))
        nan = np.isnan(ref).any(1)
        assert nan.tolist() == [False, False, True]
        worst = np.abs(ref[~nan] - dev[~nan]).max(0)
        assert (worst[[0, 2, 3, 4]] <= 1e-13).all() and worst[1] <= 1e-12, (form, kw, worst)


@FORM
def test_sequence_score(form):
    from scanpaths_amd.utils.evaltools import sequence_score as S
    paths, pairs = FORMS[form]
    K = len(paths)
    groups = [k % 2 for k in range(K)]
    clusters = S.meanshift_clusters([paths[-3], paths[-1]], bandwidth=40.0)            # the 64 points; the 5 points
    for got, P in zip(clusters, (paths[-3], paths[-1])):
        for a, b in zip(got, SR.meanshift(P, 40.0)):
            _same(a, b, (form, "mean shift"))
    strings = S.cluster_strings(paths, groups, clusters)
    for k in range(K):
        _same(strings[k], SR.labels_of(paths[k], clusters[groups[k]][0]), (form, "string", k))
    got = S.sequence_scores_pairs(strings, pairs, gap=-0.25)
    want = SR.score_pairs(strings, pairs, SR.METRICS, -0.25)
    for m in SR.METRICS:
        _same(got[m], want[m], (form, m))
    # the whole chain in one batch: every scanpath human, one cluster group
    keyed = S.keyed_sequence_scores(paths, [0] * K, [0] * K, pairs, 1, bandwidth=40.0)
    cen = SR.meanshift(np.concatenate(paths, 0), 40.0)[0]
    want = SR.score_pairs([SR.labels_of(p, cen) for p in paths], pairs)
    for m in SR.METRICS:
        _same(keyed[m], want[m], (form, "keyed", m))


@pytest.mark.parametrize("tempbin", [0.0, 50.0])
def test_scanmatch_sequences(tempbin):
    from scanpaths_amd.utils.evaltools.scanmatch import ScanMatch
    paths, pairs = FORMS["plain"]
    paths = [p * np.array([1.0, 1.0, 1000.0]) for p in paths]                          # durations in ms
    sm = ScanMatch(Xres=320, Yres=240, Xbin=16, Ybin=12, Offset=(0, 0), TempBin=tempbin, Threshold=3.5)
    seq, lens = sm.sequences(paths)
    want = [SO.fixation_to_sequence(p, 320, 240, 16, 12, (0, 0), tempbin) for p in paths]
    assert lens.cpu().tolist() == [len(w) for w in want]
    for k, w in enumerate(want):
        _same(seq[k, :len(w)].cpu().numpy(), w, ("sequence", k))
    got = sm.match_pairs(seq, lens, seq, lens, torch.tensor(pairs, dtype=torch.int32)).cpu().numpy()
    S = SO.submatrix(16, 12, 3.5)
    assert got.tolist() == [SO.nw_score(want[a], want[b], S, 0.0) for a, b in pairs]
    with pytest.raises(ValueError, match="empty"):
        sm.sequences(FORMS["empty first"][0])


@FORM
@pytest.mark.parametrize("weight", ["count", "duration"])
def test_fixation_maps(form, weight):
    from scanpaths_amd.utils.evaltools.saliency_maps import fixation_maps
    paths, _ = FORMS[form]
    paths = [p.copy() for p in paths]
    paths[-1][0, 0] = 320.0                                            # on the right edge: outside the frame
    groups = [k % 3 for k in range(len(paths))]
    maps, dropped = fixation_maps(paths, groups, (240, 320), weight=weight)
    want, wdrop = np.zeros((3, 240, 320)), np.zeros(3, dtype=np.int32)
    for p, q in zip(paths, groups):
        inside = (p[:, 0] >= 0) & (p[:, 0] < 320.0) & (p[:, 1] >= 0) & (p[:, 1] < 240.0)
        wdrop[q] += int((~inside).sum())
        p = p[inside]
        col = np.minimum(np.floor((p[:, 0] * 320) / 320.0).astype(np.int64), 319)
        row = np.minimum(np.floor((p[:, 1] * 240) / 240.0).astype(np.int64), 239)
        np.add.at(want[q], (row, col), 1.0 if weight == "count" else p[:, 2])
    _same(maps.cpu().numpy(), want, (form, weight))
    _same(dropped.cpu().numpy(), wdrop, (form, weight, "dropped"))
    assert wdrop.sum() == 1 and want.sum() > 0
